"""Small scenes named for the shape they force into the reference's mesh trees (FlatTreeBuilder of hiprz_host.cpp, restated in
oracle/rz_oracle.c), for tests/test_tree_shapes_oracle.py and tests/test_tree_shapes_gpu.py.  Same interface as generated_scenes:
`world(name)` -> (World, RenderConfig), deterministic; `flat_scene(name)` builds once.  The shapes come from geometry through the normal
flatten(), no node is edited by hand; `tree_stats` is a pure-Python walk over flat.nodes and SHAPES names what each scene must contain.

How the shapes are forced.  A triangle whose box is as large as the node's box in ANY axis is "too large" for that node; a node with both
kinds becomes a Size node (ptype 3) whose children both inherit its box: the smaller ones go to the first child, the too-large ones to
the second, where nothing is left to split, so the second child is a leaf WHATEVER its count.  `_big_leaf_mesh(n)` is a 5 x 4 grid of
quads (40 small triangles) plus n triangles that each span the mesh's whole box in x, y and z (two opposite corners of the box and a
third vertex inside): one Size node at the root, the grid in ordinary leaves, one depth-1 leaf of exactly n.  n spanning triangles alone
have nothing to split at the root: a root leaf of n, above the root limit of 32.  A Size node's children are never Size nodes themselves
(the first child holds only triangles smaller than the same box, the second is a leaf), so one mesh cannot have Size nodes at depths 0, 1
and 2: `size_chain` has two meshes, one with Size nodes at depths 0 and 2 and one whose root splits by a plane, with Size nodes at depth 1.

Every scene exists with lights (its name) and without (name + "_sky": the sky emits): a spot light and a direct light, LightSampling(2, 1),
in front of the mesh, a receiver behind it that fills the frame, so the shadow rays of a wave cross the mesh's box together.

Shape table (tree_stats of the flattened scene, both builders; asserted through SHAPES).  Leaf counts are those of non-root leaves above
8; every scene also holds the receiver's root leaf of 2.

  scene                 frame   Size nodes (depths)   non-root leaves > 8     root leaves > 8   deepest leaf   empty leaves
  big_leaf_N            48x32   1 (0)                 N                       -                 4              0
    N = 9 12 13 16 17 33 63 64 65 100 256 257 300; big_leaf_12 is 33x33; odd N: two instances, the second mirrored (9 17 63 257) or strongly non-uniform (13 33 65)
  partial_tile          5x3     1 (0)                 17                      -                 4              0
  root_leaf_N           48x32   0                     -                       N                 0              0
    N = 33 48 49 300; world of 3 instances (one leaf)
  root_leaves_world9    48x32   0                     -                       33 48 49 300      0              0      10 instances
  ties_across_chunks    48x32   1 (0)                 100                     -                 4              0
    the triangle at leaf position 5 is listed again at positions 13 and 69: emitter, mirror, diffuse
  size_chain            48x32   5 (0, 1, 2, 3)        10                      -                 4              0      two meshes
  deep                  48x32   1 (0)                 13 (at depth 21)        -                 21             0
  empty_leaf            48x32   1 (0)                 39 (at depth 32)        -                 32             31
  masks_65, masks_257   48x32   1 (0)                 65 / 257                -                 4              0      lights only

`deep`: centroids x = 8^-k, k = 0 .. 40, and 12 more on the last one.  The running mean of a geometric progression lies just below
its one or two largest terms, which are peeled off into a leaf of 1 or 2, level after level: depth 21 by the progression alone, where
the 13 triangles with one and the same centroid end in a leaf whatever their count (no centroid below the mean).  The triangle whose
box is the mesh's whole extent in y and z is too large at the root, hence the one Size node.  Each triangle is 0.62 times the size of
the one before: only the first few can be seen, and those lie far apart in x.  (A first version kept all of them large.  Beyond k = 7
two of them are nearer to each other than an ulp of the hit distance, and which one a walk reports then depends on its tree's boxes —
a box test may refuse a leaf whose triangle is nearer by a rounding — so rebuilt trees gave other last bits of the first-hit depth on
38 to 204 of 1 536 pixels, with 0 far and 0 discrete segments and every case on the reference trees exact.  test_tree_shapes_oracle.py shows the
mechanism with the reference's own box and triangle tests on two such triangles.  Rays that cross the
mesh's box near x = 0 still test the boxes of all 21 levels; hits that deep are rare, and `empty_leaf` is the scene whose 39 visible
triangles sit at depth 32.)

`empty_leaf` COULD be built, and it brings the depth-limit leaf with it.  The builder picks the split axis by the variance of the
centroids and falls back to z without asking whether any centroid lies below z's running mean.  39 tilted triangles whose boxes are
centred on z = 1 exactly, but for one on the next float above: the running mean rounds to 1, no centroid is below it, yet z has the
largest variance; one x centroid below x's mean keeps the node from ending as a leaf (x's variance is smaller, y's is 0).  So the first
half is empty, the second holds all 39 under a box cut at z = 1, and one level down the same happens again: 31 empty leaves at depths
2 .. 32, and at depth 32 > kMaxDepth = 31 the leaf of all 39, 31 above the limit of 8.  (A 40th triangle, as large as the mesh's box,
makes the root a Size node and the chain start at depth 1.  Such a chain has 2 nodes per level: a mesh of fewer than 33 triangles
would exceed the 2 T + 1 nodes that flatten() allows a mesh tree, and be refused.)
"""
import math
from collections import Counter

import numpy as np

from rayzath_amd import _abi
from rayzath_amd.engine import LightSampling, RenderConfig, Tracing
from rayzath_amd.scene import Camera, DirectLight, Instance, Material, Mesh, SpotLight, TextureBuffer, World, generate_plane

HP = math.pi / 2
PASSES = 8
BIG = (9, 12, 13, 16, 17, 33, 63, 64, 65, 100, 256, 257, 300)
ROOT = (33, 48, 49, 300)
TIE_POSITIONS = (5, 13, 69)            # k, k + 8, k + 64 of the 100-leaf
HALF = (1.0, 1.0, 0.5)                 # the big-leaf mesh's box is [-HALF, HALF]
F32 = np.float32


def _grid():
    """5 x 4 quads in the plane z = 0.3 of the box: 40 small triangles"""
    xs, ys = np.linspace(-0.9, 0.9, 6), np.linspace(-0.9, 0.9, 5)
    vertices = [(x, y, 0.3 + 0.05 * ((i + j) % 3)) for j, y in enumerate(ys) for i, x in enumerate(xs)]
    tris = []
    for j in range(4):
        for i in range(5):
            a = j * 6 + i
            tris += [(a, a + 1, a + 7), (a, a + 7, a + 6)]
    return vertices, tris


def _spanning(rng, n):
    """n triangles that each reach both ends of the box in x, y and z: one of the box's four space diagonals and a third vertex inside,
    so that they lie staggered in depth and overlap in every projection"""
    out = []
    for _ in range(n):
        sx, sy = (1.0, -1.0)[int(rng.integers(2))], (1.0, -1.0)[int(rng.integers(2))]
        a = (-sx * HALF[0], -sy * HALF[1], -HALF[2])
        b = (sx * HALF[0], sy * HALF[1], HALF[2])
        c = tuple(float(rng.uniform(-h, h)) for h in HALF)
        out.append((a, b, c) if rng.random() < 0.5 else (b, a, c))     # both facings
    return out


def _mesh(small, spanning, materials, texcrds=False, name="tree shape"):
    """`small` = (vertices, triangles) listed first, then the `spanning` triangles (three points each) with material slot materials[k]"""
    vertices, tris = list(small[0]), list(small[1])
    mats = [0] * len(tris)
    for k, t in enumerate(spanning):
        tris.append(tuple(range(len(vertices), len(vertices) + 3)))
        vertices += list(t)
        mats.append(materials[k])
    extra = {}
    if texcrds:   # the vertex's (x, y) as its texture coordinate
        extra = dict(texcrds=[((v[0] + 1) * 0.5, (v[1] + 1) * 0.5) for v in vertices], tri_texcrds=tris)
    return Mesh(vertices, tris, tri_materials=mats, name=name, **extra)


def _slots(rng, n):
    return [int(s) for s in rng.choice(np.array([0, 0, 0, 1, 2]), size=n)]      # diffuse mostly; some mirrors and emitters


def _big_leaf_mesh(n, seed, texcrds=False):
    rng = np.random.default_rng([20261018, seed])
    return _mesh(_grid(), _spanning(rng, n), _slots(rng, n) if not texcrds else [3] * n, texcrds, name=f"grid and {n} spanning")


def _root_leaf_mesh(n, seed):
    rng = np.random.default_rng([20261019, seed])
    return _mesh(([], []), _spanning(rng, n), _slots(rng, n), name=f"{n} spanning")


def _ties_mesh():
    rng = np.random.default_rng([20261020, 0])
    spanning, slots = _spanning(rng, 100), [0] * 100
    k, k8, k64 = TIE_POSITIONS
    # in front of the others over most of its area: from the front lower corner to the back upper one, third vertex in the front face
    spanning[k] = ((-1.0, -1.0, -0.5), (1.0, 1.0, 0.5), (1.0, -1.0, -0.5))
    spanning[k8] = spanning[k64] = spanning[k]
    slots[k], slots[k8], slots[k64] = 2, 1, 0                                   # emitter, mirror, diffuse
    for i, t in enumerate(spanning):                                           # the others keep behind it: third vertex in the back half
        if i not in TIE_POSITIONS:
            spanning[i] = (t[0], t[1], (t[2][0], t[2][1], abs(t[2][2]) * 0.9 + 0.05))
    return _mesh(_grid(), spanning, slots, name="ties")


def _soup(rng, n, centre, half, size):
    """n triangles with boxes of about `size` (per axis) somewhere in centre +- half"""
    out = []
    for _ in range(n):
        p = np.asarray(centre) + rng.uniform(-1, 1, 3) * (np.asarray(half) - np.asarray(size) * 0.5)
        d = [rng.uniform(-0.5, 0.5, 3) * np.asarray(size) for _ in range(3)]
        out.append(tuple(tuple(float(x) for x in p + q) for q in d))
    return out


def _corners(centre, half):
    """two triangles over the box centre +- half, each spanning it in x, y and z"""
    c, h = np.asarray(centre, float), np.asarray(half, float)
    lo, hi = c - h, c + h
    return [(tuple(lo), tuple(hi), (hi[0], lo[1], c[2])), ((lo[0], hi[1], lo[2]), (hi[0], lo[1], hi[2]), (lo[0], lo[1], c[2]))]


def _shifted(tris, scale, offset):
    return [tuple(tuple(float(p[a] * scale[a] + offset[a]) for a in range(3)) for p in t) for t in tris]


def _size_chain_meshes():
    """[nested, side by side].  nested: 10 triangles over the whole box (too large at the root: a Size node at depth 0); the others
    split by the plane x = mean at depth 1, and in each half 6 triangles as long as that half in x (too large at depth 2: Size nodes
    there) among small ones.  side by side: two such clusters apart in x, shifted against each other in y and z so that nothing is as
    large as the root's box in any axis: the root splits by a plane, and each cluster's long triangles, which reach a little past
    the plane, are too large for its half: Size nodes at depth 1."""
    rng = np.random.default_rng([20261021, 0])
    whole, halves, apart = _spanning(rng, 10), [], []
    for cx in (-0.5, 0.5):
        halves += _shifted(_spanning(rng, 6), (0.5, 0.9, 0.9), (cx, 0.0, 0.0))
        halves += _soup(rng, 14, (cx, 0, 0), (0.45, 0.5, 0.3), (0.2, 0.3, 0.15))
    nested = _mesh(([], []), halves + whole, [0] * len(halves) + _slots(rng, len(whole)), name="nested size classes")
    for side in (-1.0, 1.0):
        apart += _shifted(_spanning(rng, 5 + int(side > 0)), (0.95, 0.9, 0.9), (0.85 * side, 0.1 * side, 0.05 * side))
        apart += _soup(rng, 12, (0.9 * side, 0.1 * side, 0.05 * side), (0.7, 0.5, 0.3), (0.25, 0.3, 0.15))
    return [nested, _mesh(([], []), apart, _slots(rng, len(apart)), name="size classes side by side")]


DEEP_RATIO, DEEP_STEPS, DEEP_CLUSTER = 8.0, 40, 12


def _deep_mesh():
    """Triangle k stands across the x axis at x = DEEP_RATIO^-k: half of a rectangle centred on the axis (its box is centred on
    (x, 0, 0) exactly: the centroids differ in x alone), 0.62 times the size of the one before, and DEEP_CLUSTER more on the last
    one.  Only the first few are large enough to be seen, and those lie far apart in x: beyond k = 7 two of them are nearer to each
    other than one ulp of a hit distance, and which of two such triangles a walk reports depends on the boxes of its tree (a box test
    may refuse a leaf whose triangle is nearer by a rounding), so they are kept too small to be met by any ray but a few."""
    tris = []
    ks = list(range(DEEP_STEPS + 1)) + [DEEP_STEPS] * DEEP_CLUSTER
    for i, k in enumerate(ks):
        x = F32(DEEP_RATIO) ** F32(-k)
        s = x * F32(0.25)
        theta = math.radians(35.0 + 20.0 * ((i * 7) % 11) / 11)
        r = F32(0.8 * 0.62 ** min(i, 60))
        c, sn, side = r * F32(math.cos(theta)), r * F32(math.sin(theta)), F32((-1.0, 1.0)[i % 2])
        tris.append(((x - s, -c, -sn), (x + s, c, sn), (x, side * c, -side * sn)))
    return _mesh(([], []), tris, [0, 0, 2, 0, 1, 0] + [0] * (len(tris) - 6), name="geometric progression")


def _empty_leaf_mesh():
    """see the module docstring: 39 tilted triangles with boxes centred on (0, 0, 1) exactly, but one on z = 1 + 2^-23 and one half an
    ulp below x = 0, and a 40th as large as the mesh's box in x, y and z"""
    tris = []
    for k in range(39):
        a, b, h = F32(2.0 ** -10) * F32(1 + k), F32(0.25 + 0.015 * k), F32(2.0 ** -4) * F32(1 + k % 7) / F32(8)
        lo_x, hi_z = -a, F32(1) + h
        if k == 38:
            hi_z = np.nextafter(np.nextafter(hi_z, F32(2)), F32(2))             # box centre 1 + one ulp of 1
        if k == 20:
            lo_x = np.nextafter(lo_x, F32(-1))                                  # box centre below 0 by half an ulp of a
        tris.append(((lo_x, -b, F32(1) - h), (a, -b, hi_z), (F32(0), b, F32(1) + h * F32(0.5))))
    a, b, h = F32(2.0 ** -10) * F32(64), F32(1.0), F32(2.0 ** -4) * F32(4)
    tris.append(((-a, -b, F32(1) - h), (a, -b, F32(1) + h), (F32(0), b, F32(1))))
    return _mesh(([], []), tris, [0] * 39 + [1], name="centroids on one plane")


def _transparent_map():
    rng = np.random.default_rng([20261023, 0])
    bitmap = rng.integers(60, 256, size=(8, 8, 4), dtype=np.uint8)
    bitmap[..., 3] = rng.choice(np.array([0, 255, 128, 40, 200], np.uint8), size=(8, 8))
    return TextureBuffer(bitmap, scale=(3.0, 2.0), filter_mode="point", address_mode="wrap")


BASES = ([f"big_leaf_{n}" for n in BIG] + ["partial_tile"] + [f"root_leaf_{n}" for n in ROOT] +
         ["root_leaves_world9", "ties_across_chunks", "size_chain", "deep", "empty_leaf"])
MASKS = ("masks_65", "masks_257")
NAMES = tuple(BASES) + tuple(b + "_sky" for b in BASES) + MASKS
FRAMES = {"big_leaf_12": (33, 33), "partial_tile": (5, 3)}


def world(name):
    """(World, RenderConfig) of scene `name`"""
    assert name in NAMES, name
    base, lights = (name[:-4], False) if name.endswith("_sky") else (name, True)
    index = (BASES + list(MASKS)).index(base)
    w = World()
    w.material = Material((200, 220, 255, 0), 0.0, 0.0, 0.0 if lights else 1.5, 1.0, 0.0, name="sky")
    diffuse = w.add(Material((230, 200, 180, 255), 0.0, 1.0, name="diffuse"))
    mirror = w.add(Material.mirror())
    emitter = w.add(Material((255, 240, 200, 255), 0.0, 1.0, emission=6.0, name="emitter"))
    slots = [diffuse, mirror, emitter]
    position, scales, rotation = (0.0, 0.0, 0.0), [(1.5, 1.3, 1.0)], (0.1, 0.25, 0.05)
    if base.startswith("big_leaf_") or base == "partial_tile" or base in MASKS:
        n = 17 if base == "partial_tile" else int(base.rsplit("_", 1)[1])
        if base in MASKS:
            slots = slots + [w.add(Material((255, 255, 255, 120), 0.0, 0.6, ior=1.0, texture=_transparent_map(), name="partly transparent"))]
        meshes = [_big_leaf_mesh(n, index, texcrds=base in MASKS)]
        if n % 2:     # a second instance of the mesh: mirrored, or strongly non-uniform
            scales = [(1.2, 1.3, 1.0), (0.3, 1.6, 2.4) if [m for m in BIG if m % 2].index(n) % 2 else (-0.9, 1.1, 0.8)]
    elif base.startswith("root_leaf_"):
        meshes = [_root_leaf_mesh(int(base.rsplit("_", 1)[1]), index)]
        scales = [(1.2, 1.3, 1.0), (-0.8, 1.0, 1.2)]
    elif base == "root_leaves_world9":
        meshes = [_root_leaf_mesh(n, index + n) for n in ROOT]
        scales = [(0.8, 0.7, 0.9), (-0.7, 0.8, 0.6), (0.5, 0.9, 1.2)]
    elif base == "ties_across_chunks":
        meshes, rotation = [_ties_mesh()], (0.0, 0.1, 0.0)
    elif base == "size_chain":
        meshes, scales = _size_chain_meshes(), [(1.3, 1.2, 1.0), (0.8, 1.0, 1.0)]
    elif base == "deep":   # seen along the mesh's x axis, from the large end and from the small end
        meshes, scales, rotation = [_deep_mesh()], [(2.0, 2.4, 2.4), (2.0, -2.0, 2.6)], (0.0, HP - 0.1, 0.0)
    else:
        meshes, position, scales, rotation = [_empty_leaf_mesh()], (0.0, 0.0, -1.0), [(12.0, 1.6, 1.0)], (0.0, 0.3, 0.0)
    meshes = [w.add(m) for m in meshes]
    count = max(len(meshes), len(scales)) if base != "root_leaves_world9" else 9
    for k in range(count):
        offset = ((k + 1) // 2) * (1.3 if k % 2 else -1.3) if count > 1 else 0.0
        if count > 2:
            offset *= 0.55
        w.add(Instance(meshes[k % len(meshes)], slots, position=(position[0] + offset, position[1] + 0.1 * (k % 3), position[2] + 0.35 * (k % 4)),
                       rotation=(rotation[0], rotation[1] + 0.2 * k, rotation[2]), scale=scales[k % len(scales)], name=f"{base} {k}"))
    w.add(Instance(w.add(generate_plane(4, 6.0, 6.0)), [diffuse], position=(0, 0, 2.5), rotation=(HP, 0, 0), name="receiver"))
    if lights:   # both in front of the mesh, to the sides: their shadow rays from the receiver cross the mesh's box, some grazing its triangles
        w.add(SpotLight(position=(-1.6, 1.8, -3.0), direction=(1.4, -1.6, 5.0), color=(255, 250, 240, 255), size=0.3, emission=80.0, beam_angle=0.9))
        w.add(DirectLight(direction=(-0.35, -0.3, 1.0), color=(240, 240, 255, 255), emission=4.0, angular_size=0.1))
    width, height = FRAMES.get(base, (48, 32))
    w.camera = Camera(position=(0.0, 0.0, -3.2), rotation=(0, 0, 0), resolution=(width, height), fov=1.3, near_far=(1e-2, 1e3),
                      focal_distance=3.2, aperture=0.01, exposure_time=1.0 / 60.0)
    return w, RenderConfig(LightSampling(2, 1), Tracing(4, 8), seed=20261018 + index)


def tree_stats(flat):
    """A walk over the mesh trees of `flat` (every instance's blas_root once): dict(size_nodes, size_depths (set), leaves (Counter of
    the triangle counts of non-root leaves), leaf_depths ({count: set of depths}), root_leaves (list of counts), deepest_leaf,
    empty_leaves, size_first_inner (a Size node whose first child is an inner node))"""
    out = dict(size_nodes=0, size_depths=set(), leaves=Counter(), leaf_depths={}, root_leaves=[], deepest_leaf=0, empty_leaves=0, size_first_inner=False)
    nodes = flat.nodes
    for root in sorted({int(i["blas_root"]) for i in flat.instances}):
        todo = [(root, 0)]
        while todo:
            index, depth = todo.pop()
            meta, begin = int(nodes[index]["meta"]), int(nodes[index]["begin"])
            if meta & _abi.NODE_LEAF:
                count = meta & _abi.NODE_COUNT_MASK
                out["deepest_leaf"] = max(out["deepest_leaf"], depth)
                out["empty_leaves"] += count == 0
                if depth == 0:
                    out["root_leaves"].append(count)
                else:
                    out["leaves"][count] += 1
                    out["leaf_depths"].setdefault(count, set()).add(depth)
                continue
            if (meta >> _abi.NODE_PTYPE_SHIFT) & 3 == 3:
                out["size_nodes"] += 1
                out["size_depths"].add(depth)
                out["size_first_inner"] |= not int(nodes[begin]["meta"]) & _abi.NODE_LEAF
            todo += [(begin + 1, depth + 1), (begin, depth + 1)]
    return out


def leaf_positions(flat, mesh_triangles):
    """{triangle's index in its mesh: (leaf's node index, position in the leaf)} for the first instance's mesh, for the listed triangles"""
    nodes, out = flat.nodes, {}
    todo = [int(flat.instances[0]["blas_root"])]
    while todo:
        index = todo.pop()
        meta, begin = int(nodes[index]["meta"]), int(nodes[index]["begin"])
        if meta & _abi.NODE_LEAF:
            for p in range(meta & _abi.NODE_COUNT_MASK):
                source = int(flat.tris[begin + p]["source_index"])
                if source in mesh_triangles:
                    out[source] = (index, p)
        else:
            todo += [begin, begin + 1]
    return out


def _big(n):
    return lambda s: s["size_nodes"] == 1 and s["size_depths"] == {0} and s["leaves"][n] == 1 and s["leaf_depths"][n] == {1} and s["size_first_inner"]


def _root(*counts):
    return lambda s: sorted(c for c in s["root_leaves"] if c > 8) == sorted(counts) and s["size_nodes"] == 0


# base name -> predicate(tree_stats): what the scene must contain (with lights and without)
SHAPES = {
    **{f"big_leaf_{n}": _big(n) for n in BIG},
    "partial_tile": _big(17),
    **{f"root_leaf_{n}": _root(n) for n in ROOT},
    "root_leaves_world9": _root(*ROOT),
    "ties_across_chunks": _big(100),
    "size_chain": lambda s: s["size_depths"] >= {0, 1, 2} and s["size_first_inner"] and any(c > 8 for c in s["leaves"]),
    "deep": lambda s: s["deepest_leaf"] >= 20,
    "empty_leaf": lambda s: s["empty_leaves"] >= 1 and s["deepest_leaf"] == 32 and s["leaf_depths"].get(39) == {32},
    "masks_65": _big(65),
    "masks_257": _big(257),
}

_CACHE = {}


def flat_scene(name):
    """(FlatScene, hiprz_camera, hiprz_config, World, RenderConfig) of scene `name`, built once"""
    if name not in _CACHE:
        from rayzath_amd.scene import camera_struct, flatten
        w, config = world(name)
        _CACHE[name] = (flatten(w), camera_struct(w.camera), config.struct(), w, config)
    return _CACHE[name]
