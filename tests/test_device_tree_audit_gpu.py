"""The mesh trees the device builds, refits and rebuilds (rayzath_amd/csrc/hiprz_build.hip), downloaded and held to exact numpy references.

Frames cannot see most tree mistakes — a tree decides what a ray meets, not what it hits — so these tests read the trees themselves:

  * every mesh of the sweep (tree_sweep.py: triangle counts at the chunk edges of the kernels, ties, flat axes, runs of equal keys, far
    clusters, copies of one triangle, the awkward meshes) passes tree_audit.audit: exact boxes, leaf sizes, tiling, the side rule;
  * every mesh of more than 4 triangles IS its reference tree (tree_reference.py: the builders restated in numpy float32) — the same
    triangle order, the same nodes, partition types and child order.  Left out of that comparison, and named here, are only the meshes
    in AUDIT_ONLY_SAH under the SAH builder: a node of more than 32 coincident centres below the root is cut in half, which the reference
    marks as order-dependent (the device halves by triangle index, rz_sah_partition_kernel); they get the audit, which holds the halving
    rule and the leaf size.
    ("40 copies" is halved at the root only, where the run still stands in triangle order: it is compared.)
  * hiprz_update_triangles over ranges that start inside one mesh and end inside a later one refits exactly the meshes it touches and
    keeps topology and order; hiprz_rebuild_trees builds the reference's tree over the order and the refitted box the device holds.

The references take about 1.3 s (Morton) and 4.1 s (SAH) for the whole sweep on one CPU core; they are computed once per process."""
import numpy as np
import pytest

from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct
import tree_audit
import tree_reference
from tree_sweep import deformed_sweep, sweep, sweep_references

pytestmark = pytest.mark.gpu
DEVICE, DEVICE_SAH = 2, 3   # HIPRZ_TREE_DEVICE (Morton order), HIPRZ_TREE_DEVICE_SAH (binned surface-area build)
KIND = {DEVICE: tree_audit.MORTON, DEVICE_SAH: tree_audit.SAH}
AUDIT_ONLY_SAH = ("200 copies", "300 copies")


def _audit_only(entry, kind):
    return kind == tree_audit.SAH and entry.name.split(" #")[0] in AUDIT_ONLY_SAH


def _upload(flat, tree, devices=0):
    world = sweep()[0]
    c = Context(devices)
    c.set_tree(tree)
    c.upload_scene(flat), c.upload_camera(camera_struct(world.camera)), c.set_config(RenderConfig(tracing=Tracing(6, 4)).struct())
    return c


def _download(ctx, flat):
    nodes, _, _, roots, refpos = ctx.download_trees(len(flat.instances), len(flat.tris), len(flat.tlas_order))
    return nodes, roots, refpos.astype(np.int64)


def _frames_equal_a_fresh_upload(ctx, flat):
    fresh = _upload(flat, 0)
    for c in (ctx, fresh):
        c.render(1), c.render(3)
    assert np.array_equal(ctx.read_accum(), fresh.read_accum()) and np.array_equal(ctx.read_depth(), fresh.read_depth())
    sa, sb = ctx.read_state(), fresh.read_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    fresh.close()


def _check_built(nodes, roots, refpos, table, current, kind, reference, before_refpos, small_mode):
    """Audit of every mesh and the exact comparison with reference(entry).  `current`: the triangles in uploaded order with the vertices the
    device holds; `before_refpos`: the device order the build started from.  Returns (findings, meshes compared, meshes audited only)."""
    findings, compared, audited_only = [], [], []
    dev_tris = current[refpos]
    for e in table:
        root = int(roots[e.instance])
        mine = refpos[e.first:e.first + e.n]
        if sorted(mine.tolist()) != list(range(e.first, e.first + e.n)):
            findings.append(f"{e.name}: the mesh's range does not hold the mesh's triangles")
            continue
        if e.n <= 4:   # never built: the uploaded single leaf
            findings += [f"{e.name}: {f}" for f in tree_audit.audit(nodes, root, dev_tris, kind, e.first, e.n, mode=small_mode)]
            continue
        findings += [f"{e.name}: {f}" for f in tree_audit.audit(nodes, root, dev_tris, kind, e.first, e.n)][:4]
        if _audit_only(e, kind):
            audited_only.append(e.name)
            continue
        where = np.empty(e.n, dtype=np.int64)   # uploaded position -> index before the build
        where[before_refpos[e.first:e.first + e.n] - e.first] = np.arange(e.n)
        ref = reference(e)
        if ref.order_dependent:
            findings.append(f"{e.name}: the reference itself depends on the order of a halved run, the mesh cannot be compared")
        findings += [f"{e.name}: {f}" for f in tree_reference.differences(ref, nodes, root, where[mine - e.first], e.first)]
        compared.append(e.name)
    return findings, compared, audited_only


@pytest.mark.parametrize("device,devices", [(DEVICE, 0), (DEVICE_SAH, 0), (DEVICE_SAH, [0, 0])])
def test_first_build_is_the_reference_tree(built, device, devices):
    _, flat, table = sweep()
    kind = KIND[device]
    refs = sweep_references(kind)
    assert all(refs[e.name].order_dependent == _audit_only(e, kind) for e in table if e.n > 4)
    ctx = _upload(flat, device, devices)
    assert ctx.tree() == device
    nodes, roots, refpos = _download(ctx, flat)
    findings, compared, audited_only = _check_built(nodes, roots, refpos, table, flat.tris, kind, lambda e: refs[e.name], np.arange(len(flat.tris)), "enclose")
    print(kind, "compared exactly:", len(compared), "audit only:", audited_only)
    assert not findings, "\n".join(findings[:40])
    assert len(compared) + len(audited_only) == sum(e.n > 4 for e in table) and len(audited_only) == (2 if kind == tree_audit.SAH else 0)
    # (the comparison reads what THIS builder built: held to the other builder's reference, the largest mesh is another tree)
    other = sweep_references(tree_audit.SAH if kind == tree_audit.MORTON else tree_audit.MORTON)
    e = max(table, key=lambda e: e.n)
    assert tree_reference.differences(other[e.name], nodes, int(roots[e.instance]), refpos[e.first:e.first + e.n] - e.first, e.first)
    ctx.close()


@pytest.mark.parametrize("devices", [0, [0, 0]])
def test_halved_meshes_are_the_reference_tree_at_every_upload(built, devices):
    """The meshes of AUDIT_ONLY_SAH under the SAH builder, in three fresh contexts: a node that no plane separates is halved by triangle
    index, which is what tree_reference.sah_tree does (its `ix` ascends), so the device's tree IS the reference — the same triangle
    order, nodes, partition types and child order — whatever the wave scheduling was."""
    _, flat, table = sweep()
    refs = sweep_references(tree_audit.SAH)
    halved = [e for e in table if _audit_only(e, tree_audit.SAH)]
    assert len(halved) >= 2 and all(refs[e.name].order_dependent for e in halved)
    findings = []
    for upload in range(3):
        ctx = _upload(flat, DEVICE_SAH, devices)
        nodes, roots, refpos = _download(ctx, flat)
        ctx.close()
        for e in halved:
            mine = refpos[e.first:e.first + e.n]
            assert sorted(mine.tolist()) == list(range(e.first, e.first + e.n)), e.name
            findings += [f"upload {upload} {e.name}: {f}" for f in tree_reference.differences(refs[e.name], nodes, int(roots[e.instance]), mine - e.first, e.first)][:4]
    assert not findings, "\n".join(findings[:40])


def _update_ranges(table):
    """three ranges of the uploaded order that start inside one mesh and end inside a later one (or inside the same: one single triangle),
    none a multiple of 256 long, then everything"""
    at = {e.name.split(" #")[0]: e for e in table}
    ranges = [(at["sweep soup 33"].first + 7, at["sweep soup 256"].first + 131),
              (at["grid 1024"].first + 513, at["grid 1024"].first + 514),
              (at["sweep soup 4096"].first + 1000, at["grid 4097"].first + 3)]
    assert all((b - a) % 256 for a, b in ranges)
    total = table[-1].first + table[-1].n
    return ranges + [(0, total)]


@pytest.mark.parametrize("device", [DEVICE, DEVICE_SAH])
def test_refits_over_ranges_that_cut_through_meshes(built, device):
    _, flat0, table = sweep()
    flat1, new_tris, new_attrs = deformed_sweep()
    kind = KIND[device]
    ctx = _upload(flat0, device)
    nodes, roots, refpos = _download(ctx, flat0)
    before = {e.name: tree_audit.snapshot(nodes, int(roots[e.instance]), refpos, e.first, e.n) for e in table}
    slots = {e.name: [row[0] for row in tree_audit._collect(nodes, int(roots[e.instance]), [])] for e in table}
    current = flat0.tris.copy()
    findings = []
    ranges = _update_ranges(table)
    for a, b in ranges + ranges[-1:]:   # the last call twice in a row: the arrival counters start from zero again
        ctx.update_triangles(a, new_tris[a:b], new_attrs[a:b])
        current[a:b] = new_tris[a:b]
        after, roots_after, refpos_after = _download(ctx, flat0)
        assert np.array_equal(roots_after, roots)
        dev_tris = current[refpos_after]
        for e in table:
            if e.first < b and a < e.first + e.n:
                findings += [f"[{a}, {b}) {e.name}: {f}" for f in tree_audit.audit(after, int(roots[e.instance]), dev_tris, kind, e.first, e.n, mode="refit",
                                                                               before=before[e.name], refpos=refpos_after)][:4]
            elif not np.array_equal(after[slots[e.name]], nodes[slots[e.name]]):
                findings.append(f"[{a}, {b}) {e.name}: an untouched mesh's nodes changed")
        nodes = after
    assert not findings, "\n".join(findings[:40])
    ctx.update_instances(flat1.instances)
    _frames_equal_a_fresh_upload(ctx, flat1)
    ctx.close()


@pytest.mark.parametrize("builder", [DEVICE, DEVICE_SAH])
def test_rebuild_over_the_deformed_vertices_is_the_reference_tree(built, builder):
    """The reference is built over the order the device holds before the rebuild and over the refitted root box — a rebuild that kept
    the box of the first upload would sort the triangles on a stale grid."""
    _, flat0, table = sweep()
    flat1, new_tris, new_attrs = deformed_sweep()
    kind = KIND[builder]
    ctx = _upload(flat0, DEVICE_SAH)
    ctx.update_triangles(0, new_tris, new_attrs)
    ctx.update_instances(flat1.instances)
    nodes0, roots0, refpos0 = _download(ctx, flat0)
    dev_tris0 = new_tris[refpos0]
    ctx.rebuild_trees(builder)
    assert ctx.tree() == builder
    nodes, roots, refpos = _download(ctx, flat0)
    build = {tree_audit.MORTON: tree_reference.morton_tree, tree_audit.SAH: tree_reference.sah_tree}[kind]
    def reference(e):
        box = nodes0[int(roots0[e.instance])]
        return build(dev_tris0[e.first:e.first + e.n], box["bb_min"], box["bb_max"])
    findings, compared, audited_only = _check_built(nodes, roots, refpos, table, new_tris, kind, reference, refpos0, "built")
    print(kind, "compared exactly after the rebuild:", len(compared), "audit only:", audited_only)
    assert not findings, "\n".join(findings[:40])
    # a stale grid is visible here: the refitted boxes differ from the uploaded ones for every built mesh, and a reference that bins
    # over the uploaded box is another tree than the device's
    assert all(not np.array_equal(nodes0[int(roots0[e.instance])]["bb_min"], flat0.nodes[e.root]["bb_min"]) for e in table if e.n > 4)
    e = next(e for e in table if e.name.startswith("sweep soup 4096"))
    stale = build(dev_tris0[e.first:e.first + e.n], flat0.nodes[e.root]["bb_min"], flat0.nodes[e.root]["bb_max"])
    where = np.empty(e.n, dtype=np.int64)
    where[refpos0[e.first:e.first + e.n] - e.first] = np.arange(e.n)
    assert tree_reference.differences(stale, nodes, int(roots[e.instance]), where[refpos[e.first:e.first + e.n] - e.first], e.first)
    _frames_equal_a_fresh_upload(ctx, flat1)
    ctx.close()
