"""Worlds for the surface records (rayzath_amd/csrc/hiprz_scene_host.hpp: pack_surface_section): what tests/test_surface_records.py packs
on the host and tests/test_surface_records_gpu.py renders.  Every world is small enough to be staged in LDS and has at most a few dozen
triangles per mesh; the frames are 64 x 48 unless a case says otherwise."""
import math

import numpy as np

from rayzath_amd import scenes
from rayzath_amd.scene import (Camera, Instance, Material, Mesh, SpotLight, TextureBuffer, World, generate_cube, generate_plane,
                               generate_sphere)

HP = math.pi / 2


def camera(width=64, height=48, position=(0, 1, -3.5), rotation=(0, 0, 0)):
    return Camera(position=position, rotation=rotation, resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=0.02, exposure_time=1.0 / 60.0)


def cornell(width=64, height=48):
    """config B's world (the camera inside the room)"""
    return scenes.cornell_box(width, height)


def cornell_from_behind(width=64, height=48):
    """the camera behind the back wall, looking into the room: the open wall meshes are hit on their other side first"""
    world = scenes.cornell_box(width, height)
    world.camera = camera(width, height, position=(0.3, 1.2, 4.5), rotation=(0, math.pi, 0))
    return world


def _materials(world):
    return [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror()),
            world.add(Material((200, 60, 40, 255), 0.1, 0.6, name="red"))]


def _floor_and_lamp(world, mats):
    w = 3.0 * math.sqrt(2.0)
    plane = world.add(generate_plane(4, w, w))
    world.add(Instance(plane, [mats[0]], position=(0, -1, 0), name="floor"))
    world.add(Instance(plane, [mats[1]], position=(0, 3.2, 0), scale=(0.4, 1.0, 0.4), name="lamp"))
    return plane


def placements(width=64, height=48):
    """a non-uniform scale, a mirrored instance (one negative scale component), and two instances of one mesh under different placements"""
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    cube = world.add(generate_cube())
    world.add(Instance(cube, [mats[3]], position=(-1.4, -0.2, 0.8), rotation=(0.2, 0.5, 0.1), scale=(1.5, 0.5, 2.5), name="non-uniform"))
    world.add(Instance(cube, [mats[2]], position=(0.2, 0.0, 1.2), rotation=(0.1, -0.4, 0.3), scale=(-1.0, 1.2, 0.8), name="mirrored"))
    world.add(Instance(cube, [mats[0]], position=(1.5, -0.3, 0.2), rotation=(0.0, 0.9, 0.0), scale=(0.7, 1.4, 0.7), name="shared a"))
    world.add(Instance(cube, [mats[3]], position=(1.1, 1.6, 1.0), rotation=(0.6, 0.2, 0.4), scale=(0.9, 0.3, 0.6), name="shared b"))
    world.camera = camera(width, height)
    return world


def vertex_normals(width=64, height=48):
    """a sphere with vertex normals (48 triangles, an inner root: the mapped normal is interpolated per hit, the normal comes from the
    record) between planes"""
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    sphere = world.add(generate_sphere(8, normals=True, texture_coordinates=True))
    world.add(Instance(sphere, [mats[2]], position=(-0.6, 0.3, 0.6), rotation=(0.3, 0.2, 0.0), scale=(1.3, 0.9, 1.1), name="sphere"))
    world.add(Instance(sphere, [mats[3]], position=(1.0, 0.0, 0.2), scale=(0.8, 0.8, 0.8), name="sphere 2"))
    world.camera = camera(width, height)
    return world


def normal_mapped(width=64, height=48):
    """a textured quad under a material with a normal map (normal from the record, mapped normal from the map) beside a textured cube
    without one"""
    rng = np.random.default_rng(5)
    tex = np.concatenate([rng.integers(60, 256, size=(16, 16, 3), dtype=np.uint8), np.full((16, 16, 1), 255, np.uint8)], axis=-1)
    n = rng.integers(-40, 41, size=(16, 16, 2))
    nrm = np.stack([128 + n[..., 0], 128 + n[..., 1], np.full((16, 16), 255), np.full((16, 16), 255)], axis=-1).astype(np.uint8)
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    mapped = world.add(Material((255, 255, 255, 255), 0.3, 0.4, texture=TextureBuffer(tex), normal_map=TextureBuffer(nrm), name="mapped"))
    plain = world.add(Material((255, 255, 255, 255), 0.0, 0.8, texture=TextureBuffer(tex), name="textured"))
    quad = world.add(generate_plane(4, 1.2, 1.2))
    world.add(Instance(quad, [mapped], position=(-0.8, 0.8, 1.2), rotation=(HP * 0.8, 0.2, 0.0), scale=(1.0, 1.0, 1.4), name="normal-mapped quad"))
    world.add(Instance(world.add(generate_cube()), [plain], position=(1.0, -0.3, 0.6), rotation=(0, 0.5, 0), name="textured cube"))
    world.camera = camera(width, height)
    return world


def degenerate_mesh():
    """a quad whose second triangle has no area (two equal corners) followed by a proper one"""
    v = [(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)]
    return Mesh(v, [(0, 2, 1), (0, 0, 3), (0, 3, 2)], name="quad with a zero-area triangle")


def extreme_cubes(width=64, height=48):
    """a zero-area triangle and cubes scaled by 3e19 and 1e-20 in one component: the faces across the scaled axis get flagged records
    (the host's arithmetic leaves the normal numbers there), the other faces valid ones.  For the packer only: a box of 3e19 takes the
    slab tests of the walks out of the finite numbers, where the staged and the unstaged walks do not agree with or without records
    (56 pixels of this frame differ between them on either library)."""
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    cube = world.add(generate_cube())
    world.add(Instance(world.add(degenerate_mesh()), [mats[3]], position=(0.0, 0.2, 1.0), rotation=(HP * 0.7, 0, 0), name="degenerate"))
    world.add(Instance(cube, [mats[0]], position=(0.0, 2.0, 1.5), scale=(3.0e19, 0.4, 0.4), name="scale 3e19"))
    world.add(Instance(cube, [mats[2]], position=(-1.2, 0.5, 0.5), rotation=(0, 0.3, 0), scale=(1.0e-20, 1.5, 1.5), name="scale 1e-20"))
    world.add(Instance(cube, [mats[3]], position=(1.3, -0.4, 0.4), rotation=(0, 0.4, 0), name="plain cube"))
    world.camera = camera(width, height)
    return world


def extremes(width=64, height=48):
    """a zero-area triangle, and quads scaled by 3e19 and 5e-20 ACROSS their plane: the geometry is what it is at scale 1 (every vertex has
    y = 0), the records of both quads are flagged (the normal's y / scale squared is subnormal, or overflows) and their hits compute as
    before, in waves whose other lanes read the valid records of the floor, the lamp and a cube.  5e-20 and not less: from 3e-20 down
    the ray taken into the quad's space overflows inside the walks, and the staged and the unstaged walks — the two sides of the GPU
    test's comparison — stop agreeing on a few pixels with or without records (1e-20: 9 pixels of this frame on either library)."""
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    quad = world.add(generate_plane(4, 1.0, 1.0))
    world.add(Instance(world.add(degenerate_mesh()), [mats[3]], position=(0.0, 0.2, 1.0), rotation=(HP * 0.7, 0, 0), name="degenerate"))
    world.add(Instance(quad, [mats[0]], position=(-1.3, 1.2, 1.4), rotation=(HP * 0.9, 0.3, 0), scale=(1.0, 3.0e19, 1.2), name="scale 3e19"))
    world.add(Instance(quad, [mats[2]], position=(1.2, 1.4, 1.0), rotation=(HP * 0.8, -0.4, 0.1), scale=(0.9, 5.0e-20, 1.0), name="scale 5e-20"))
    world.add(Instance(world.add(generate_cube()), [mats[3]], position=(1.3, -0.4, 0.4), rotation=(0, 0.4, 0), name="plain cube"))
    world.camera = camera(width, height)
    return world


def material_slots(width=64, height=48):
    """triangles whose material slot is inside the instance's table, unset (-1 is what flatten writes for None), beyond the table, and
    beyond the 64 slots an instance can have"""
    world = World()
    mats = _materials(world)
    _floor_and_lamp(world, mats)
    cube = generate_cube()
    slots = [0, 0, 1, 1, 2, 2, 3, 3, 9, 9, 70, 200]
    mesh = world.add(Mesh(cube.vertices, cube.tri_vertices, texcrds=cube.texcrds, tri_texcrds=cube.tri_texcrds, tri_materials=slots, name="slots"))
    world.add(Instance(mesh, [mats[3], mats[2], None, mats[0]], position=(-0.8, 0.0, 0.8), rotation=(0.3, 0.6, 0.0), scale=(1.4, 1.4, 1.4), name="four slots"))
    world.add(Instance(mesh, [mats[1]], position=(1.0, 0.2, 0.4), rotation=(0.1, -0.5, 0.2), name="one slot"))
    world.camera = camera(width, height)
    return world


def spot_lit(width=64, height=48):
    """the Cornell room under a spot light: the shading variant with next-event estimation"""
    world = scenes.cornell_box(width, height)
    world.add(SpotLight(position=(0.5, 2.6, -0.5), direction=(-0.2, -1.0, 0.4), color=(255, 240, 220, 255), size=0.15, emission=80.0, beam_angle=1.0))
    return world
