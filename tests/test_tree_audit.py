"""tree_audit.py and tree_reference.py proved on the CPU, before the device trees are held to them (test_device_tree_audit_gpu.py):

  * both references build every mesh of the sweep (tree_sweep.py); every tree passes the audit and, packed into a snapshot, the host's
    scene validation (every index in range, every walk ends, the leaves tile the meshes);
  * the SAH reference's trees cost less than the snapshot's reference trees wherever a mesh has more than 64 triangles — the bar the host's
    SAH builder meets in test_tree_rebuild.py;
  * mutants: each mistake the audit and the comparison exist for, made to a reference tree or its triangle order at one small and one
    large mesh, is reported."""
import ctypes as C

import numpy as np
import pytest

from rayzath_amd import _abi, _lib
from rayzath_amd.scene import FlatScene, Mesh
import tree_audit
import tree_reference
from tree_audit import MORTON, SAH
from tree_reference import RefNode, RefTree
from tree_sweep import sweep, sweep_references
from test_tree_rebuild import sah_cost

BUILD = {MORTON: tree_reference.morton_tree, SAH: tree_reference.sah_tree}


def _reference_scene(kind):
    """the sweep snapshot with every mesh tree replaced by its reference tree: (FlatScene, {mesh name: root slot})"""
    _, flat, table = sweep()
    refs = sweep_references(kind)
    n_world = min(e.root for e in table)
    parts, order, roots, new_root = [flat.nodes[:n_world]], np.arange(len(flat.tris)), flat.instances["blas_root"].copy(), {}
    cursor = n_world
    for e in table:
        ref = refs.get(e.name) or RefTree(np.arange(e.n), RefNode(0, e.n))   # 4 triangles or fewer: the one leaf they are uploaded as
        order[e.first:e.first + e.n] = e.first + ref.order
        parts.append(tree_reference.pack_nodes(ref, flat.tris[order[e.first:e.first + e.n]], cursor, e.first))
        new_root[e.name] = cursor
        roots[flat.instances["blas_root"] == e.root] = cursor
        cursor += len(parts[-1])
    inst = flat.instances.copy()
    inst["blas_root"] = roots
    snap = FlatScene(nodes=np.concatenate(parts), tlas_root=flat.tlas_root, tlas_order=flat.tlas_order, tris=flat.tris[order], tri_attrs=flat.tri_attrs[order],
                     instances=inst, inst_materials=flat.inst_materials, materials=flat.materials, textures=flat.textures, texels=flat.texels,
                     spot_lights=flat.spot_lights, direct_lights=flat.direct_lights)
    return snap, new_root


@pytest.mark.parametrize("kind", [MORTON, SAH])
def test_reference_trees_pass_the_audit_and_the_hosts_validation(kind):
    _, flat, table = sweep()
    snap, roots = _reference_scene(kind)
    refs = sweep_references(kind)
    for e in table:
        assert tree_audit.audit(snap.nodes, roots[e.name], snap.tris, kind, e.first, e.n) == [], e.name
        if e.n > 4:   # ... and the comparison finds a reference tree equal to itself, read back from its node records
            assert tree_reference.differences(refs[e.name], snap.nodes, roots[e.name], refs[e.name].order, e.first) == [], e.name
    msg = C.create_string_buffer(256)
    assert _lib.load().hiprz_validate_scene(C.byref(snap.struct), msg, 256) == _abi.OK, msg.value


def test_sah_reference_trees_cost_less_than_the_snapshots():
    _, flat, table = sweep()
    snap, roots = _reference_scene(SAH)
    big = [e for e in table if e.n > 64]
    assert len(big) >= 20
    coincident = 0
    for e in big:
        cost = sah_cost(snap.nodes, roots[e.name])
        mn, mx = tree_reference.triangle_boxes(flat.tris[e.first:e.first + e.n])
        if (mn == mn[0]).all() and (mx == mx[0]).all():
            # Copies of one triangle: every node has the root's area, so ANY tree costs 1.2 * inner nodes + triangles, and the snapshot's
            # tree — one leaf of all of them, which no builder with leaves of at most 8 may emit — costs exactly the triangles.  "Less"
            # is out of reach by arithmetic; what holds instead is the exact figure.
            inner = sum(1 for n in sweep_references(SAH)[e.name].walk() if n.kids)
            assert sah_cost(flat.nodes, e.root) == e.n and abs(cost - (1.2 * inner + e.n)) < 1e-9 * cost, e.name
            coincident += 1
            continue
        assert cost < sah_cost(flat.nodes, e.root), e.name
    assert coincident == 2   # "200 copies" and "300 copies"


# ---------------------------------------------------------------- mutants
class Case:
    """one mesh before a build, its reference tree and the tree's node records (root in slot 0, triangles from position 0)"""

    def __init__(self, kind, tris, lo, hi):
        self.kind, self.tris, self.lo, self.hi = kind, tris, np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        self.ref = BUILD[kind](tris, lo, hi)
        self.order, self.nodes = self.ref.order.copy(), tree_reference.pack_nodes(self.ref, tris[self.ref.order])

    def use(self, tree):
        self.order, self.nodes = tree.order.copy(), tree_reference.pack_nodes(tree, self.tris[tree.order])

    def reports(self):
        audit = tree_audit.audit(self.nodes, 0, self.tris[self.order], self.kind, 0, len(self.tris))
        return audit, tree_reference.differences(self.ref, self.nodes, 0, self.order)


def _sweep_case(kind, name):
    _, flat, table = sweep()
    e = next(e for e in table if e.name.split(" #")[0] == name)
    return Case(kind, flat.tris[e.first:e.first + e.n], flat.nodes[e.root]["bb_min"], flat.nodes[e.root]["bb_max"])


def _mesh_case(kind, mesh):
    from rayzath_amd.scene import HostBackend
    nodes, tris, _ = HostBackend().mesh_tree(mesh)
    return Case(kind, tris, nodes[0]["bb_min"], nodes[0]["bb_max"])


def _some_inner_node(case, want=lambda node: True):
    """slot of an inner node in the middle of the table"""
    inner = [k for k in range(len(case.nodes)) if not case.nodes[k]["meta"] & tree_audit.LEAF and want(k)]
    assert inner
    return inner[len(inner) // 2]


def _ulp(case, field, direction):
    k = _some_inner_node(case)
    case.nodes[k][field][1] = np.nextafter(case.nodes[k][field][1], np.float32(direction * np.inf))


def grown_box(case):
    _ulp(case, "bb_max", +1)
    return "audit"


def shrunk_box(case):
    _ulp(case, "bb_min", +1)
    return "audit"


def children_swapped(case):
    k = _some_inner_node(case)
    b = int(case.nodes[k]["begin"])
    case.nodes[[b, b + 1]] = case.nodes[[b + 1, b]]
    return "audit"


def wrong_partition_type(case):
    k = _some_inner_node(case, lambda k: (int(case.nodes[k]["meta"]) >> 29) & 3 != 3)
    ptype = (int(case.nodes[k]["meta"]) >> 29) & 3
    case.nodes[k]["meta"] = ((ptype + 1) % 3) << 29
    return "audit" if case.kind == MORTON else "either"


def _exchange(case, p, q):
    """the triangles at positions p and q change places; the boxes are fitted exactly again (the grouping is wrong, not the boxes)"""
    order = case.ref.order.copy()
    order[[p, q]] = order[[q, p]]
    case.use(RefTree(order, case.ref.root))


def triangles_exchanged_between_sibling_leaves(case):
    n = next(n for n in case.ref.walk() if n.kids and not n.kids[0].kids and not n.kids[1].kids)
    _exchange(case, n.kids[0].first, n.kids[1].first)
    return "comparison"


def equal_key_triangles_exchanged(case):
    keys = tree_reference.morton_keys(case.tris, case.lo, case.hi)[case.ref.order]
    p = int(np.flatnonzero(keys[1:] == keys[:-1])[0])
    _exchange(case, p, p + 1)
    return "comparison"


def plane_moved_by_one_bin(case):
    case.use(tree_reference.sah_tree(case.tris, case.lo, case.hi, root_plane_shift=1))
    return "comparison"


def morton_subtree_of_four_left_uncollapsed(case):
    assert any(n.count == 4 for n in case.ref.walk())
    case.use(tree_reference.morton_tree(case.tris, case.lo, case.hi, keep_four=True))
    return "audit"


def key_on_a_grid_one_ulp_off(case):
    case.use(tree_reference.morton_tree(case.tris, np.nextafter(case.lo, np.float32(np.inf)), case.hi))
    return "comparison"


def sah_leaf_of_nine(case):
    """the builder run with leaves of up to 9 where that gives one, else a subtree of 9 triangles collapsed by hand"""
    tree = tree_reference.sah_tree(case.tris, case.lo, case.hi, leaf_max=9)
    if any(n.count == 9 and not n.kids for n in tree.walk()):
        case.use(tree)
        return "audit"
    rows = tree_audit._collect(case.nodes, 0, [])
    slot, first, count = min(((s, f, c) for s, f, c, p, _ in rows if p >= 0 and c >= 9), key=lambda r: r[2])
    assert count == 9
    case.nodes[slot]["begin"], case.nodes[slot]["meta"] = first, tree_audit.LEAF | count
    return "audit"


def _nine_copies(kind):
    one = np.array([[-0.3, -0.2, 0.0], [0.3, -0.2, 0.1], [0.0, 0.3, -0.1]], np.float32)
    return _mesh_case(kind, Mesh(np.tile(one, (9, 1)), np.arange(27, dtype=np.uint32).reshape(-1, 3)))


def _on_cell_borders(planes):
    """Pairs of triangles standing in planes x = const of a mesh box -1 .. 1: the first of a pair exactly on a border of the 1024 Morton
    cells (its centroid's x is the plane's, exactly), the second half a cell below it.  On the true grid the second sorts first; on a
    grid that starts one ulp higher both fall into the lower cell and the stable sort keeps the first in front."""
    def mesh(kind):
        x = np.repeat(np.arange(planes + 1, dtype=np.float32) * np.float32(2.0 / planes) - np.float32(1.0), 2)
        x[1::2] -= np.float32(1.0 / 1024.0)
        x[1] = x[0]   # (nothing lies below the box)
        yz = np.array([[0.0, 0.0], [0.1, 0.0], [0.0, 0.1]], np.float32)
        v = np.concatenate([np.repeat(x, 3)[:, None], np.tile(yz, (len(x), 1))], 1)
        return _mesh_case(kind, Mesh(v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)))
    return mesh


MUTANTS = [   # (the change, builder, the small mesh, the large mesh)
    (grown_box, MORTON, "sweep soup 33", "sweep soup 4097"), (grown_box, SAH, "sweep soup 33", "sweep soup 4097"),
    (shrunk_box, MORTON, "sweep soup 33", "sweep soup 4097"), (shrunk_box, SAH, "sweep soup 33", "sweep soup 4097"),
    (children_swapped, MORTON, "sweep soup 33", "sweep soup 4097"), (children_swapped, SAH, "sweep soup 33", "sweep soup 4097"),
    (wrong_partition_type, MORTON, "sweep soup 33", "sweep soup 4097"), (wrong_partition_type, SAH, "sweep soup 33", "sweep soup 4097"),
    (triangles_exchanged_between_sibling_leaves, MORTON, "sweep soup 33", "sweep soup 4097"),
    (triangles_exchanged_between_sibling_leaves, SAH, "sweep soup 33", "sweep soup 4097"),
    (equal_key_triangles_exchanged, MORTON, "40 copies", "duplicates 1025"),
    (plane_moved_by_one_bin, SAH, "sweep soup 65", "sweep soup 4096"),
    (morton_subtree_of_four_left_uncollapsed, MORTON, "sweep soup 33", "sweep soup 4097"),
    (key_on_a_grid_one_ulp_off, MORTON, _on_cell_borders(16), _on_cell_borders(1024)),
    (sah_leaf_of_nine, SAH, _nine_copies, "sweep soup 4097"),
]


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("mutant,kind,small,large", MUTANTS, ids=[f"{m.__name__}-{k}" for m, k, _, _ in MUTANTS])
def test_mutants_are_reported(mutant, kind, small, large, size):
    mesh = small if size == "small" else large
    case = mesh(kind) if callable(mesh) else _sweep_case(kind, mesh)
    assert case.reports() == ([], [])   # sound before the change
    by = mutant(case)
    audit, comparison = case.reports()
    assert audit or comparison
    if by == "audit":
        assert audit, comparison
    if by == "comparison":
        assert comparison, audit


@pytest.mark.parametrize("kind", [MORTON, SAH])
def test_refit_and_enclose_modes_report_what_they_are_for(kind):
    """What the device tests rely on after hiprz_update_triangles and for the uploaded single leaves: moved vertices under the old boxes,
    a changed topology and a changed order are reported in refit mode; enclose mode accepts a loose box and refuses a tight one."""
    case = _sweep_case(kind, "sweep soup 257")
    n, refpos = len(case.tris), case.order.copy()
    tris = case.tris[case.order]
    before = tree_audit.snapshot(case.nodes, 0, refpos, 0, n)
    refit = lambda nodes, t=tris, r=refpos: tree_audit.audit(nodes, 0, t, kind, 0, n, mode="refit", before=before, refpos=r)
    assert refit(case.nodes) == []
    moved = tris.copy()
    moved["v2"][n // 2] += np.float32(3.0)   # one vertex leaves every box above it
    assert any("exact box" in f for f in refit(case.nodes, moved))
    assert refit(tree_reference.pack_nodes(case.ref, moved), moved) == []   # ... and fitted again, the same topology is sound
    swapped = case.nodes.copy()
    b = int(swapped[_some_inner_node(case)]["begin"])
    swapped[[b, b + 1]] = swapped[[b + 1, b]]
    assert refit(swapped) == []   # a refit does not assert the side rule: swapped children hold the same (first, count, type) set
    collapsed = case.nodes.copy()
    rows = tree_audit._collect(collapsed, 0, [])
    slot, first, count = next((s, f, c) for s, f, c, p, _ in rows if p >= 0 and c <= (4 if kind == MORTON else 8) + 2)
    collapsed[slot]["begin"], collapsed[slot]["meta"] = first, tree_audit.LEAF | count
    assert "the refit changed the topology" in refit(collapsed)
    other = refpos.copy()
    other[[0, 1]] = other[[1, 0]]
    assert "the refit changed the triangle order" in refit(case.nodes, tris, other)
    leaf = tree_reference.pack_nodes(RefTree(np.arange(3), RefNode(0, 3)), tris[:3])
    enclose = lambda nodes: tree_audit.audit(nodes, 0, tris[:3], kind, 0, 3, mode="enclose")
    assert enclose(leaf) == []
    loose, tight = leaf.copy(), leaf.copy()
    loose[0]["bb_max"] += np.float32(1.0)
    tight[0]["bb_max"][2] = np.nextafter(tight[0]["bb_max"][2], np.float32(-np.inf))
    assert enclose(loose) == [] and tree_audit.audit(loose, 0, tris[:3], kind, 0, 3) != []
    assert enclose(tight) != []
