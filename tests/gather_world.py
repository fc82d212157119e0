"""The world of tests/test_gather_gpu.py and its atlas, with the float64 geometry the tests hold the device to: the floor, cube and sphere
of tests/test_light_gpu.py (rebuilt here) plus one wall, a 64 x 48 atlas in which floor, cube and wall each have a rectangle of their own
and the sphere has none (the cube's six faces each in a cell of their own inside the cube's rectangle), the world-space triangles in float64, a float64 closest hit over them (for the CPU check of the boundary cap in
tests/test_gather_reference.py) and the float64 barycentrics of a known hit.

THE WALL is the unit plane stood upright, 2.1 wide and 1.4 tall, in front of the back third of the floor with its front to the camera and
the lights: floor points behind it see its back, floor points before it gather its colour."""
import numpy as np

from rayzath_amd import atlas
from rayzath_amd.scene import (Camera, DirectLight, Instance, Material, Mesh, SpotLight, World, flatten, generate_cube, generate_plane, generate_sphere)

F = np.float32
W, H = 64, 48
FLOOR, CUBE, SPHERE, WALL = 0, 1, 2, 3
# (u0, v0, u1, v1) in atlas units: the mesh's own UVs, which lie in [0, 1]^2, are scaled into the rectangle.  No edge of a rectangle lies on
# a texel boundary of a 64 x 48 atlas.
RECTS = {FLOOR: (0.03, 0.04, 0.47, 0.96), CUBE: (0.53, 0.04, 0.97, 0.46), WALL: (0.53, 0.54, 0.97, 0.96)}
# The cube's six faces (f = triangle // 2) each have a cell of their own, 3 x 2 in the cube's rectangle, with a gutter between cells given
# here as a share of the rectangle: 0.1 x 28.16 = 2.8 texels across and 0.14 x 20.16 = 2.8 texels down at 64 x 48, more than the two rings
# of dilation the tests use, so that a ring-1 texel next to a cell holds that cell's face.  No edge of a cell lies within 0.05 texel of a
# texel boundary or of a texel centre of a 64 x 48 atlas (tests/test_bake_meaning.py).
CELLS, GUTTER = (3, 2), (0.1, 0.14)
SPOT = dict(position=(1.5, 4.0, -1.0), direction=(-0.3, -1.0, 0.25), color=(255, 240, 220, 255), size=0.35, emission=60.0, beam_angle=0.8)
DIRECT = dict(direction=(-0.25, -1.0, 0.45), color=(255, 255, 240, 255), emission=4.0, angular_size=0.15)


def world(moved=False, geometry=True, lights=True):
    w = World()
    if geometry:
        grey = w.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
        w.add(Instance(w.add(generate_plane(4, 1.0, 1.0)), [grey], position=(0, 0, 0), scale=(5, 1, 5), name="floor"))
        w.add(Instance(w.add(generate_cube()), [grey], position=(1.1, 1.2, 0.6) if moved else (0.2, 1.2, 0.0), rotation=(0.3, 0.5, 0.1), scale=(1.2, 0.6, 1.2), name="cube"))
        w.add(Instance(w.add(generate_sphere(8)), [grey], position=(-1.6, 0.5, -0.8), scale=(0.5, 0.5, 0.5), name="sphere"))
        plane = w.add(generate_plane(4, 1.0, 1.0))
        for turn in (0.5 * np.pi, -0.5 * np.pi):          # whichever way round the rotation goes: the wall's front (the plane's +y) faces -z
            wall = Instance(plane, [grey], position=(-1.0, 0.75, 1.0), rotation=(turn, 0.0, 0.0), scale=(1.5, 1.0, 1.0), name="wall")
            w.instances.append(wall)
            if flatten(w).instances[WALL]["y_axis"][2] < -0.9:
                break
            w.instances.pop()
        else:
            raise AssertionError("neither rotation turns the wall's front to -z")
    if lights:
        w.add(SpotLight(**SPOT))
        w.add(DirectLight(**DIRECT))
    w.camera = Camera(position=(0.5, 3.5, -6.0), resolution=(32, 24), fov=1.0, near_far=(1e-2, 1e3))
    w.camera.look_at((0.0, 0.5, 0.0))
    return w


def cube_cell(face):
    """(u0, v0, u1, v1) of a cube face's cell in the unit square the cube's rectangle scales: column face % 3, row face // 3"""
    c, r = face % CELLS[0], face // CELLS[0]
    cw, ch = (1.0 - (CELLS[0] - 1) * GUTTER[0]) / CELLS[0], (1.0 - (CELLS[1] - 1) * GUTTER[1]) / CELLS[1]
    return c * (cw + GUTTER[0]), r * (ch + GUTTER[1]), c * (cw + GUTTER[0]) + cw, r * (ch + GUTTER[1]) + ch


def parts(w, overlapping=False):
    """the atlas's parts: floor, cube and wall, each mesh's own UVs scaled into its rectangle; the sphere is left out on purpose.  The cube's
    own UVs lay every face over the whole unit square, so each face f = triangle // 2 is first scaled into its own cell (cube_cell): no
    texel is claimed twice.  overlapping=True leaves the cube's UVs as they are: six faces on the same texels, of which the lowest id
    owns each (include/hiprz_atlas.h), so that five faces read the first one's texels."""
    out = []
    for instance, (u0, v0, u1, v1) in RECTS.items():
        tris = atlas.charts(w.instances[instance].mesh)
        for k in (1, 2, 3):
            assert (tris[f"u{k}"] >= 0).all() and (tris[f"u{k}"] <= 1).all() and (tris[f"v{k}"] >= 0).all() and (tris[f"v{k}"] <= 1).all()
        if instance == CUBE and not overlapping:
            assert len(tris) == 2 * CELLS[0] * CELLS[1]
            cell = np.array([cube_cell(t // 2) for t in range(len(tris))], F)
            for k in (1, 2, 3):
                tris[f"u{k}"], tris[f"v{k}"] = cell[:, 0] + (cell[:, 2] - cell[:, 0]) * tris[f"u{k}"], cell[:, 1] + (cell[:, 3] - cell[:, 1]) * tris[f"v{k}"]
        for k in (1, 2, 3):
            tris[f"u{k}"], tris[f"v{k}"] = F(u0) + F(u1 - u0) * tris[f"u{k}"], F(v0) + F(v1 - v0) * tris[f"v{k}"]
        out.append((instance, tris))
    return out


def inward_box():
    """a cube mesh whose triangles are wound the other way: its front faces look inward, a closed room"""
    cube = generate_cube()
    return Mesh(cube.vertices, cube.tri_vertices[:, ::-1].copy(), texcrds=cube.texcrds, tri_texcrds=cube.tri_texcrds[:, ::-1].copy(), name="inward box")


def square_below(a, h):
    """a square of side 2a at height h, parallel to the floor, its front looking down"""
    v = [(-a, h, -a), (a, h, -a), (a, h, a), (-a, h, a)]
    t = [(0, 0), (1, 0), (1, 1), (0, 1)]
    tv = [(0, 1, 2), (0, 2, 3)]
    return Mesh(v, tv, texcrds=t, tri_texcrds=tv, name="radiant square")


def world_triangles(w, flat):
    """per instance i: (T, 3, 3) float64 world-space vertices of the mesh's triangles in the mesh's own order, placed as the flat scene's
    instance record places them: p * scale, turned by the axes, moved by the position (include/hiprz_atlas.h "THE POINT")"""
    out = []
    for i, inst in enumerate(w.instances):
        rec = flat.instances[i]
        position, scale = rec["position"].astype(np.float64), rec["scale"].astype(np.float64)
        xa, ya, za = (rec[k].astype(np.float64) for k in ("x_axis", "y_axis", "z_axis"))
        q = inst.mesh.vertices.astype(np.float64)[inst.mesh.tri_vertices] * scale
        out.append(q[..., 0:1] * xa + q[..., 1:2] * ya + q[..., 2:3] * za + position)
    return out


def barycentrics(tri, origin, direction):
    """Moeller-Trumbore in float64 for rays (n, 3) against their own triangle (n, 3, 3): (t, bx, by, det), bx and by the weights of vertices
    2 and 3"""
    v1, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pvec = np.cross(direction, e2)
    det = np.einsum("ij,ij->i", e1, pvec)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tvec = origin - v1
        bx = np.einsum("ij,ij->i", tvec, pvec) * inv
        qvec = np.cross(tvec, e1)
        by = np.einsum("ij,ij->i", direction, qvec) * inv
        t = np.einsum("ij,ij->i", e2, qvec) * inv
    return t, bx, by, det


def closest_hits(triangles, origin, direction, near):
    """the float64 closest hit of rays (n, 3) over the triangles of world_triangles(): (instance (-1: none), triangle, bx, by, front)"""
    n = len(origin)
    best = np.full(n, np.inf)
    inst, tri_id, bx, by, front = np.full(n, -1), np.zeros(n, np.int64), np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for i, tris in enumerate(triangles):
        for k, tri in enumerate(tris):
            t, b1, b2, det = barycentrics(np.broadcast_to(tri, (n, 3, 3)), origin, direction)
            with np.errstate(invalid="ignore"):
                hit = (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > near) & (t < best)
            best = np.where(hit, t, best)
            inst[hit], tri_id[hit], bx[hit], by[hit], front[hit] = i, k, b1[hit], b2[hit], (det > 0)[hit]
    return inst, tri_id, bx, by, front


def on_a_boundary(u, v, margin):
    """the float64 UV lies within `margin` texel of a texel boundary of the W x H atlas"""
    near = lambda a: np.abs(a - np.rint(a)) < margin
    return near(u * W) | near(v * H)
