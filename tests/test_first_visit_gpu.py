"""The first visit in place of the one-leaf walk (first_visit and closest_hit_flat in hiprz_device.hpp, flat_pick_first in
hiprz_flat_pick.hpp): ahead of the binned rounds a lane whose ray's first candidate is a mesh of one leaf of at most 4 triangles
(FlatWorld::small) visits it for its own ray; a first candidate of any other kind is left to round 0.

Every case goes through test_packed_pairs_gpu.compare_with_the_stack_walk: the default traversal on pipelines 2, 0 and 1 against a twin
on the LDS-stack walk, accumulator, depth and path state bit for bit after render(1) and render(3), every counter after
render_counted(2), and the CPU oracle's exact fields.  One tile of 32x8 pixels, depth 6, unless stated.  The scenes, with what the
flattened scene and the CPU oracle's first hits say of them (asserted before anything runs on the GPU; "leaf order" = the world leaf's
slice of tlas_order, "small" = the mesh root is a leaf of at most 4 triangles):

  quads_only                six quads, all small: every first visit is in place.  A wall over the whole frame, and a small quad in front of
                            it that stands last in leaf order: for the pixels that see it, a second narrow visit through the binned rounds
  cube_first                a cube first in leaf order over part of the tile, quads behind: its lanes must not commit the pick, and
                            waves mix lanes that visit in place with lanes that wait (8 to 248 pixels whose first hit is the cube)
  all_cubes                 test_flat_walk_gpu's eight cubes: no instance is small, the walk must be the parent's
  box_hit_triangles_missed  a quad turned 45 degrees in its own plane, first in leaf order, a wall behind it: its box covers corners its
                            triangles do not, so there the visit in place finds nothing and the range stays (at least 16 pixels see the
                            wall where a quad the size of the first one's box would have been hit)
  inner_root_first          a sphere (a mesh tree with an inner root) first in leaf order: not small, through the binned rounds
  five_triangles            a leaf of exactly 4 and a leaf of exactly 5 triangles side by side: the boundary of `small`
  scaled_slabs              rotated quads with non-unit scales as first candidates of camera rays (near = 0.01): the hit in place moves
                            the near end by a rounding and the boxes are tested again
  coinciding                a quad listed twice (4 triangles) as two instances at the same place, first and second in leaf order: equal
                            distances, the first in leaf order wins
  leaf_of_three             a world leaf of 3 instances instead of 8
  partial_5x3, partial_1x1  lanes without a pixel; a wave with a single ray
  nine                      nine instances: a world tree with inner nodes, the general binned walk, which must be unaffected
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi
from rayzath_amd.engine import RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, World, camera_struct, flatten, generate_cube, generate_plane, generate_sphere
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


def wall_and(front, n_wall=5, width=32, height=8, wall_z=1.0, front_first=False):
    """a wall of n_wall quads side by side over the whole frame; front = [(mesh, position, rotation, scale)] stand before it, listed
    behind the wall or (front_first) ahead of it: the world leaf keeps the listing order"""
    world = World()
    mats = _materials(world)

    def add_front():
        for k, (mesh, position, rotation, scale) in enumerate(front):
            world.add(Instance(world.add(mesh), [mats[2 - k % 2]], position=position, rotation=rotation, scale=scale, name=f"front {k}"))

    if front_first:
        add_front()
    quad = world.add(generate_plane(4, 9.6 / n_wall, 3.0))
    for k in range(n_wall):
        world.add(Instance(quad, [mats[k % 2]], position=((k - (n_wall - 1) / 2) * 9.6 / n_wall, 1, wall_z), rotation=(HP, 0, 0), name=f"wall {k}"))
    if not front_first:
        add_front()
    world.camera = _camera(width, height)
    return world


def scaled_slabs():
    world = World()
    mats = _materials(world)
    quad = world.add(generate_plane(4, 1.0, 1.0))
    for k in range(6):   # near to far in listing order, staggered: the columns of the frame look through different sets
        world.add(Instance(quad, [mats[1] if k == 5 else mats[0] if k % 2 else mats[2]], position=(-1.2 + 0.45 * k, 1, -1.0 + 0.45 * k),
                           rotation=(HP + 0.05, 0.1, 0), scale=(1.7, 1.0, 0.6), name=f"slab {k}"))
    world.camera = _camera(32, 8)
    return world


def polygons(meshes, width=32, height=8, same_place=False):
    world = World()
    mats = _materials(world)
    n = len(meshes)
    slots = {}
    for k, mesh in enumerate(meshes):
        if id(mesh) not in slots:
            slots[id(mesh)] = world.add(mesh)
        x = 0.0 if same_place else (k - (n - 1) / 2) * 2.2
        world.add(Instance(slots[id(mesh)], [mats[k % 3]], position=(x, 1, 1.0), rotation=(HP, 0, 0), name=f"polygon {k}"))
    world.camera = _camera(width, height)
    return world


TWICE = repeated_quad(2, 2.0, 2.0)
CASES = {
    "quads_only": lambda: wall_and([(generate_plane(4, 1.0, 1.0), (0.3, 1, 0.2), (HP, 0, 0), (1, 1, 1))]),
    "cube_first": lambda: wall_and([(generate_cube(), (-1.1, 1, 0.0), (0, 0.37, 0), (0.55, 0.6, 0.5))], front_first=True),
    "all_cubes": lambda: cubes(False),
    "box_hit_triangles_missed": lambda: wall_and([(generate_plane(4, 1.6, 1.6), (0.0, 1, 0.2), (HP, 0, math.pi / 4), (1, 1, 1))], front_first=True),
    "inner_root_first": lambda: wall_and([(generate_sphere(8), (0.5, 1, 0.0), (0, 0, 0), (0.7, 0.7, 0.7))], front_first=True),
    "five_triangles": lambda: polygons([fan(4, 2.0, 2.0), fan(5, 2.0, 2.0)]),
    "scaled_slabs": scaled_slabs,
    "coinciding": lambda: polygons([TWICE, TWICE], same_place=True),
    "leaf_of_three": lambda: polygons([fan(2, 2.0, 2.0), fan(2, 1.5, 2.5), fan(2, 2.0, 1.5)]),
    "partial_5x3": lambda: wall_and([(generate_plane(4, 1.0, 1.0), (0.3, 1, 0.2), (HP, 0, 0), (1, 1, 1))], width=5, height=3),
    "partial_1x1": lambda: wall_and([(generate_plane(4, 1.0, 1.0), (0.3, 1, 0.2), (HP, 0, 0), (1, 1, 1))], width=1, height=1),
    "nine": lambda: wall_and([(generate_plane(4, 1.0, 1.0), (0.3, 1, 0.2), (HP, 0, 0), (1, 1, 1))], n_wall=8),
}


class Facts:
    """what the flattened scene and the CPU oracle's first hits say of a scene"""

    def __init__(self, world):
        self.flat, self.cam = flatten(world), camera_struct(world.camera)
        flat = self.flat
        root = flat.nodes[flat.tlas_root]
        self.one_leaf = bool(int(root["meta"]) & _abi.NODE_LEAF) and (int(root["meta"]) & _abi.NODE_COUNT_MASK) <= 8
        begin, count = int(root["begin"]), int(root["meta"]) & _abi.NODE_COUNT_MASK
        self.order = [int(i) for i in flat.tlas_order[begin:begin + count]] if self.one_leaf else []
        self.leaf, self.triangles = [], []
        for inst in flat.instances:
            meta = int(flat.nodes[int(inst["blas_root"])]["meta"])
            self.leaf.append(bool(meta & _abi.NODE_LEAF))
            self.triangles.append(meta & _abi.NODE_COUNT_MASK if meta & _abi.NODE_LEAF else None)
        self.small = [leaf and n <= 4 for leaf, n in zip(self.leaf, self.triangles)]
        hits = oracle.first_hits(flat, self.cam)
        self.hit = hits["triangle"] >= 0
        self.instance = np.where(self.hit, hits["instance"].astype(np.int64), -1)
        self.names = [inst.name for inst in world.instances]

    def index(self, name):
        return self.names.index(name)

    def pixels(self, name):
        return int((self.instance == self.index(name)).sum())


def check_quads_only(f):
    assert f.one_leaf and len(f.order) == 6 and all(f.small)
    assert f.hit.all()   # the wall covers the frame: every ray has a wall as a candidate
    assert f.order[-1] == f.index("front 0") and f.pixels("front 0") >= 8   # the second narrow visit


def check_cube_first(f):
    cube = f.index("front 0")
    assert f.one_leaf and f.order[0] == cube and f.leaf[cube] and f.triangles[cube] == 12
    assert sum(f.small) == 5 and 8 <= f.pixels("front 0") <= 248


def check_all_cubes(f):
    assert f.one_leaf and len(f.order) == 8 and not any(f.small) and f.hit.all()


def check_box_hit_triangles_missed(f):
    quad = f.index("front 0")
    assert f.one_leaf and f.order[0] == quad and all(f.small)
    # the same scene with a quad the size of the first one's box in its place: where that is hit and the turned quad is not, a ray has
    # the turned quad's box and none of its triangles
    box = f.flat.instances[quad]
    size = box["bb_max"] - box["bb_min"]
    assert size[2] < 1.0e-5 and abs(size[0] - size[1]) < 1.0e-5 and size[0] > 1.6 * 1.4
    covered = Facts(wall_and([(generate_plane(4, float(size[0]), float(size[1])), (0.0, 1, 0.2), (HP, 0, 0), (1, 1, 1))], front_first=True))
    corners = (covered.instance == covered.index("front 0")) & (f.instance != quad)
    assert f.pixels("front 0") >= 16 and int(corners.sum()) >= 16
    assert f.hit[corners].all()   # the wall behind it


def check_inner_root_first(f):
    sphere = f.index("front 0")
    assert f.one_leaf and f.order[0] == sphere and not f.leaf[sphere] and sum(f.small) == 5
    assert 8 <= f.pixels("front 0") <= 248


def check_five_triangles(f):
    assert f.one_leaf and f.triangles == [4, 5] and f.small == [True, False]
    assert f.pixels("polygon 0") >= 16 and f.pixels("polygon 1") >= 16


def check_scaled_slabs(f):
    assert f.one_leaf and len(f.order) == 6 and all(f.small)
    assert all(tuple(inst["scale"]) != (1.0, 1.0, 1.0) for inst in f.flat.instances)
    assert int(f.hit.sum()) >= 128 and len(set(f.instance[f.hit].tolist())) >= 3


def check_coinciding(f):
    assert f.one_leaf and len(f.order) == 2 and f.triangles == [4, 4]
    a, b = f.flat.instances[0], f.flat.instances[1]
    assert tuple(a["position"]) == tuple(b["position"]) and a["blas_root"] == b["blas_root"]
    assert int(f.hit.sum()) >= 16 and set(f.instance[f.hit].tolist()) == {f.order[0]}   # the first in leaf order wins


def check_leaf_of_three(f):
    assert f.one_leaf and len(f.order) == 3 and all(f.small) and int(f.hit.sum()) >= 64


def check_partial(f):
    assert f.one_leaf and len(f.order) == 6 and all(f.small) and f.hit.all()
    assert f.cam.width * f.cam.height < 64


def check_nine(f):
    assert not f.one_leaf and len(f.flat.instances) == 9


CHECKS = {"quads_only": check_quads_only, "cube_first": check_cube_first, "all_cubes": check_all_cubes,
          "box_hit_triangles_missed": check_box_hit_triangles_missed, "inner_root_first": check_inner_root_first,
          "five_triangles": check_five_triangles, "scaled_slabs": check_scaled_slabs, "coinciding": check_coinciding,
          "leaf_of_three": check_leaf_of_three, "partial_5x3": check_partial, "partial_1x1": check_partial, "nine": check_nine}


@pytest.mark.parametrize("name", list(CASES))
def test_first_visit_equals_the_stack_walk_and_the_oracle(name):
    facts = Facts(CASES[name]())
    print(name, "leaf order", facts.order, "small", facts.small, "first-hit pixels per instance",
          {n: facts.pixels(n) for n in facts.names})
    CHECKS[name](facts)
    compare_with_the_stack_walk(name, facts.flat, facts.cam, RenderConfig(tracing=Tracing(6, 8)).struct())
