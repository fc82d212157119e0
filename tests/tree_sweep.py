"""The mesh sweep of the device tree audit (test_tree_audit.py on the CPU, test_device_tree_audit_gpu.py on the device): one world that holds
every mesh once, on a Cornell box, so that one upload per builder builds them all.

Triangle counts sit at the chunk edges of the build kernels — 256-thread blocks, the 1024-wide scan over n - 1 flags, 4096-key sort tiles,
leaves of 4 (Morton) and 8 (SAH), subtrees of 32 — and the shapes at their awkward cases: exact ties and a flat axis (grid planes), two far
clusters under three mesh-spanning triangles, runs of equal keys (duplicated triangles), copies of one triangle (no plane separates
anything), plus every mesh of test_device_build_gpu._awkward_world."""
import collections
import functools

import numpy as np

from rayzath_amd import scenes
from rayzath_amd.scene import Instance, Mesh, flatten

MeshEntry = collections.namedtuple("MeshEntry", "name first n root instance")   # range in flat.tris, root slot in flat.nodes, first instance of the mesh

COUNTS = (4, 5, 8, 9, 32, 33, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 2049, 4096, 4097, 12289)


def soup(rng, n, spread=0.5):
    v = rng.uniform(-spread, spread, (n, 3, 3)).astype(np.float32) * np.float32(0.35) + rng.uniform(-spread, spread, (n, 1, 3)).astype(np.float32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def grid_plane(nx, nz, extra=0, name=None):
    """nx x nz quads of side 1/16 in the plane y = 0.25 (two triangles each; every coordinate a small dyadic fraction: exact ties in keys and
    costs, one flat axis), `extra` more triangles on the next row."""
    step = np.float32(1.0 / 16.0)
    x, z = np.meshgrid(np.arange(nx + 1, dtype=np.float32) * step - np.float32(1.0), np.arange(nz + 2, dtype=np.float32) * step - np.float32(1.0), indexing="ij")
    v = np.stack([x, np.full_like(x, 0.25), z], -1).reshape(-1, 3)
    at = lambda i, k: i * (nz + 2) + k
    t = []
    for i in range(nx):
        for k in range(nz):
            t += [(at(i, k), at(i + 1, k), at(i, k + 1)), (at(i + 1, k), at(i + 1, k + 1), at(i, k + 1))]
    for i in range(extra):
        t.append((at(i, nz), at(i + 1, nz), at(i, nz + 1)))
    t = np.array(t, dtype=np.uint32)
    used = np.unique(t)   # only the vertices in use: the mesh box is the triangles' box
    return Mesh(v[used], np.searchsorted(used, t).astype(np.uint32), name=name or f"grid {len(t)}")


def sweep_meshes():
    rng = np.random.default_rng(20)
    meshes = [Mesh(*soup(rng, n), name=f"sweep soup {n}") for n in COUNTS]
    meshes += [grid_plane(16, 32), grid_plane(32, 64, extra=1)]
    v = np.concatenate([soup(rng, 127, 0.2)[0] + np.float32([-10, 0, 1]), soup(rng, 127, 0.2)[0] + np.float32([10, 2, -1]),
                        np.float32([[-10.2, -0.3, 0.8], [10.2, 2.3, -0.8], [0, 5, 0], [-10.1, 0.2, 1.2], [10.1, 1.8, -1.2], [0, -5, 0.5],
                                    [-9.9, 0.1, 0.9], [9.9, 2.1, -0.9], [0.5, 0.5, 6]])])
    meshes.append(Mesh(v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), name="two clusters 257"))
    v, _ = soup(rng, 467)
    rows = np.concatenate([[k] * (7 if k % 5 == 0 else 1) for k in range(467)])[:1025]
    v = v.reshape(-1, 3, 3)[rows].reshape(-1, 3)
    meshes.append(Mesh(v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), name="duplicates 1025"))
    one = np.array([[-0.3, -0.2, 0.0], [0.3, -0.2, 0.1], [0.0, 0.3, -0.1]], np.float32)
    for n in (40, 300):
        meshes.append(Mesh(np.tile(one, (n, 1)), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), tri_materials=(np.arange(n) % 2).astype(np.uint32), name=f"{n} copies"))
    assert [len(m.tri_vertices) for m in meshes[len(COUNTS):]] == [1024, 4097, 257, 1025, 40, 300]
    return meshes


def sweep_world(width=96, height=60):
    from test_device_build_gpu import _awkward_world
    world = _awkward_world()
    world.camera = scenes._camera(width, height)
    paint = world.materials[-2:]
    for i, m in enumerate(sweep_meshes()):
        m = world.add(m)
        scale = 0.05 if m.name.startswith("two clusters") else 0.5
        world.add(Instance(m, paint, position=(-1.2 + 0.4 * (i % 7), -0.6 + 0.55 * (i // 7), 0.2 + 0.2 * (i % 4)), rotation=(0.15 * i, 0.4, 0.05 * i), scale=(scale,) * 3))
    return world


def deform(world):
    """every vertex of every mesh moved non-affinely"""
    seen = set()
    for inst in world.instances:
        if inst.mesh is None or id(inst.mesh) in seen:
            continue
        seen.add(id(inst.mesh))
        v = inst.mesh.vertices
        inst.mesh.vertices = np.ascontiguousarray(v * np.array([1.1, 0.9, 1.05], dtype=np.float32) + np.sin(v[:, [1, 2, 0]] * np.float32(7.0)).astype(np.float32) * np.float32(0.05), dtype=np.float32)
    return world


def mesh_table(world, flat):
    """The distinct meshes as MeshEntry, in the order flatten() lays them out in."""
    out, first, seen = [], 0, set()
    for i, inst in enumerate(world.instances):
        if inst.mesh is None or id(inst.mesh) in seen:
            continue
        seen.add(id(inst.mesh))
        n = len(inst.mesh.tri_vertices)
        out.append(MeshEntry(f"{inst.mesh.name} #{len(out)}", first, n, int(flat.instances[i]["blas_root"]), i))
        first += n
    assert first == len(flat.tris)
    return out


def records_in_order_of(flat0, flat1, table):
    """flat1's triangle records, mesh by mesh, in flat0's order (the same meshes with moved vertices: a mesh keeps its range, its
    reference tree may order the triangles differently)"""
    order = np.empty(len(flat0.tris), dtype=np.int64)
    for _, first, n, _, _ in table:
        where = np.empty(n, dtype=np.int64)
        where[flat1.tris["source_index"][first:first + n]] = np.arange(n)
        order[first:first + n] = first + where[flat0.tris["source_index"][first:first + n]]
    return flat1.tris[order], flat1.tri_attrs[order]


@functools.lru_cache(None)
def sweep():
    """(world, flat, table) of the sweep world, built once per process"""
    world = sweep_world()
    flat = flatten(world)
    return world, flat, mesh_table(world, flat)


@functools.lru_cache(None)
def deformed_sweep():
    """(flat of the deformed sweep world, its triangle and shading records in the undeformed flat's order)"""
    _, flat0, table = sweep()
    flat1 = flatten(deform(sweep_world()))
    return (flat1,) + records_in_order_of(flat0, flat1, table)


@functools.lru_cache(None)
def sweep_references(kind):
    """{mesh name: RefTree} of every sweep mesh of more than 4 triangles, built over the snapshot's order and the snapshot's mesh box"""
    import tree_reference
    _, flat, table = sweep()
    build = {"morton": tree_reference.morton_tree, "sah": tree_reference.sah_tree}[kind]
    return {e.name: build(flat.tris[e.first:e.first + e.n], flat.nodes[e.root]["bb_min"], flat.nodes[e.root]["bb_max"]) for e in table if e.n > 4}
