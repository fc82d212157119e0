"""The one-leaf walk's triangle loop on pair records (the two triangles of a pair stored interleaved behind the hot blob,
hiprz_scene_host.hpp: PackedScene::pair_section; binned_visit in hiprz_device.hpp).

Every case is a one-leaf world of at most 8 instances whose meshes are single leaves of chosen triangle counts (asserted on the flattened
scene), rendered 1 + 8 passes through three launch forms — the resident pipeline, the split pipeline, and nine render(1) calls on the
default pipeline — and each form's accumulator must equal, with np.array_equal, the frame of a twin on the LDS-stack walk
(set_traversal_mode(1)), which reads the 48-byte triangle records one by one.  Then render_counted(2): box_tests and tri_tests equal the
stack walk's.  Frames are 64 x 48 (12 tiles, more than one workgroup), one is 72 x 20 (partial tiles).

  counts_small   1, 2, 3, 4 (one lane per visit: a lone triangle, one record, a record and a half-filled one, two records) and 5, 7, 8, 9
                 (eight lanes per visit: lanes 0..2 / 0..3 / 0..3 / 0..4 hold a record, the last one of 5, 7 and 9 half filled)
  counts_large   12, 15, 16 (six, eight and eight lanes), 17 (lane 0 takes a second, half-filled record), 31 and 32 (two records in
                 every lane; 31: the last half filled)
  shared         one mesh of 9 triangles under two instances of different scale (they share records), beside a mesh of 3
  inner_root     a sphere of 48 triangles, whose root is an inner node (closest_in_mesh_stack keeps the 48-byte records; it has no pair
                 record), between single-leaf meshes of 5 and 12.  The launch plan gives a scene with such a mesh the LDS-stack walk, so
                 the three forms ask for the binned walk (set_traversal_mode(2)), which is the one-leaf walk on this world
  ties           coinciding triangles, the first in leaf order must win: every triangle of a quad listed twice in succession (equal
                 distances INSIDE one record: 4 triangles on one lane), the quad listed twice (t0 t1 t0 t1: across two records of one
                 lane), four times (8 triangles: across lanes of an octet) and nine times (18 triangles: lane 0 holds records 0 and 8,
                 across records of one lane and across lanes at once)
  mixed          `mixed` of tests/test_packed_pairs_gpu.py: most rounds on the one-lane-per-visit fallback, where one lane walks the
                 records of a 17-triangle leaf
  partial_72x20  3, 12 and 17 triangles on a frame of partial tiles

`counts_small` also goes against the CPU oracle at the project's parity bar (first-hit depth and finished-path counts equal, colours
within rel 1e-3 on all but 1 % of the pixels), and hiprz_selftest — whose kernel compares the step on a pair record's operands
(tri_pair_step) with the one-by-one loop — must report no mismatch.
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, Mesh, World, camera_struct, flatten, generate_plane, generate_sphere
from test_packed_pairs_gpu import fan, mixed, repeated_quad

pytestmark = pytest.mark.gpu

HP = math.pi / 2


def _camera(width, height):
    return Camera(position=(0, 1, -3.5), rotation=(0, 0, 0), resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=0.02, exposure_time=1.0 / 60.0)


def doubled_quad():
    """t0 t0 t1 t1: the two triangles of every pair record coincide"""
    quad = generate_plane(4, 1.0, 1.0)
    return Mesh(quad.vertices, np.repeat(quad.tri_vertices, 2, axis=0), texcrds=quad.texcrds, tri_texcrds=np.repeat(quad.tri_texcrds, 2, axis=0),
                name="quad, every triangle twice")


def grid(meshes, width, height, scales=None):
    """the meshes in rows of four facing the camera, staggered in depth so that rays that pass one meet another; white, emitter, mirror"""
    world = World()
    mats = [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror())]
    ids = {}
    for k, mesh in enumerate(meshes):
        if id(mesh) not in ids:
            ids[id(mesh)] = world.add(mesh)
        col, row = k % 4, k // 4
        cols = min(4, len(meshes) - 4 * row)
        world.add(Instance(ids[id(mesh)], [mats[k % 3]], position=((col - (cols - 1) / 2) * 1.7, 0.1 + 1.8 * row, 1.0 + 0.35 * (k % 3)),
                           rotation=(HP, 0, 0.03 * k), scale=scales[k] if scales else (1.0, 1.0, 1.0), name=f"polygon {k}"))
    world.camera = _camera(width, height)
    return world


def _shared():
    nine = fan(9)
    return grid([nine, fan(3), nine], 64, 48, scales=[(1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (0.6, 1.0, 1.3)]), [9, 3, 9]


CASES = {
    "counts_small": lambda: (grid([fan(n) for n in (1, 2, 3, 4, 5, 7, 8, 9)], 64, 48), [1, 2, 3, 4, 5, 7, 8, 9]),
    "counts_large": lambda: (grid([fan(n) for n in (12, 15, 16, 17, 31, 32)], 64, 48), [12, 15, 16, 17, 31, 32]),
    "shared": _shared,
    "inner_root": lambda: (grid([fan(5), generate_sphere(8), fan(12)], 64, 48, scales=[(1.0, 1.0, 1.0), (0.6, 0.6, 0.6), (1.0, 1.0, 1.0)]), [5, None, 12]),
    "ties": lambda: (grid([doubled_quad(), repeated_quad(2), repeated_quad(4), repeated_quad(9)], 64, 48), [4, 4, 8, 18]),
    "mixed": mixed,
    "partial_72x20": lambda: (grid([fan(3), fan(12), fan(17)], 72, 20), [3, 12, 17]),
}


def root_counts(flat):
    """per instance: the triangle count of its mesh's root when that is a leaf, else None"""
    out = []
    for inst in flat.instances:
        meta = int(flat.nodes[int(inst["blas_root"])]["meta"])
        out.append(meta & _abi.NODE_COUNT_MASK if meta & _abi.NODE_LEAF else None)
    return out


def _context(flat, cam, cfg, mode=None, pipeline=None):
    ctx = Context(0)
    if mode is not None:
        ctx.set_traversal_mode(mode)
    if pipeline is not None:
        ctx.set_pipeline(pipeline)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    return ctx


@pytest.mark.parametrize("name", list(CASES))
def test_pair_records_equal_the_stack_walk(name):
    world, want = CASES[name]()
    flat, cam = flatten(world), camera_struct(world.camera)
    root = int(flat.nodes[flat.tlas_root]["meta"])
    assert root & _abi.NODE_LEAF and (root & _abi.NODE_COUNT_MASK) == len(want) <= 8
    assert root_counts(flat) == want
    if name == "shared":
        assert flat.instances["blas_root"][0] == flat.instances["blas_root"][2] and tuple(flat.instances["scale"][0]) != tuple(flat.instances["scale"][2])
    cfg = RenderConfig(tracing=Tracing(6, 8)).struct()

    twin = _context(flat, cam, cfg, mode=1)
    twin.render(1), twin.render(8)
    want_accum = twin.read_accum()
    want_counted = twin.render_counted(2)
    assert want_counted["hits"] > 0 and want_counted["tri_tests"] > 0
    twin.close()

    mode = 2 if name == "inner_root" else None
    for label, pipeline, one_at_a_time in (("resident pipeline", 2, False), ("split pipeline", 1, False), ("one render(1) at a time", None, True)):
        ctx = _context(flat, cam, cfg, mode=mode, pipeline=pipeline)
        if one_at_a_time:
            for _ in range(9):
                ctx.render(1)
        else:
            ctx.render(1), ctx.render(8)
            assert ctx.pipeline() == pipeline
        assert np.array_equal(ctx.read_accum(), want_accum), f"{name}, {label}: accum after 1 + 8 passes differs from the stack walk"
        counted = ctx.render_counted(2)
        for key in ("box_tests", "tri_tests"):
            assert counted[key] == want_counted[key], f"{name}, {label}: {key} {counted[key]} != {want_counted[key]} (stack walk)"
        ctx.close()


def test_pair_records_against_the_oracle():
    world, _ = CASES["counts_small"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    cfg = RenderConfig(tracing=Tracing(6, 8)).struct()
    ctx = _context(flat, cam, cfg)
    ctx.render(1), ctx.render(8)
    ref = oracle.OracleRenderer(flat, cam, cfg)
    ref.render(1), ref.render(8)
    accum, depth = ctx.read_accum(), ctx.read_depth()
    ctx.close()
    assert np.array_equal(depth, ref.depth), "first-hit depth differs from the oracle"
    assert np.array_equal(accum[..., 3], ref.accum[..., 3]), "finished-path counts differ from the oracle"
    err = np.abs(accum[..., :3] - ref.accum[..., :3])
    bad = (err > 1e-3 * np.maximum(np.abs(ref.accum[..., :3]), 1.0)).any(-1).mean()
    print(f"pixels beyond rel 1e-3: {bad:.4%}")
    assert bad <= 0.01
    ref.close()


@pytest.mark.parametrize("seed", [3, 20262, 0xBADC0DE])
def test_selftest_finds_no_mismatch(seed):
    ctx = Context(0)
    bad, n = ctx.selftest(256, seed)
    ctx.close()
    assert n >= 2 * 1024 * 256 * 256
    assert bad == 0, f"seed {seed}: {bad} mismatches in {n} cases"
