"""The packer's surface section (rayzath_amd/csrc/hiprz_scene_host.cpp: pack_surface_section — what analyze_intersection reads instead of
deriving normals and material ids per hit, in the kernels that stage the scene in LDS) WITHOUT a GPU: tests/surface_records_main.cpp, a
program of its own, is compiled with the packer under AddressSanitizer and UBSan and run as a child process over scenes this file writes.
The sections it returns are compared, bit for bit, with a float32 numpy restatement of analyze_intersection's sequence for each side:

  * the ten worlds of tests/test_pair_records.py (single-leaf meshes of 1 .. 32 triangles, shared meshes, an inner root, an empty leaf,
    nine instances, a split world tree — and trees rebuilt at upload, which have no section), with face normals computed here
  * config B's world at 64 x 48: 72 records, all valid; the two sides of an axis-aligned wall are NOT each other's negation (a zero keeps
    its sign) — the reason for a record per side
  * non-uniform and mirrored instances and two instances of one mesh (records per instance); a sphere with vertex normals (normal valid,
    mapped normal not); a zero-area triangle (neither); scales of 3e19 and 1e-20 on cubes, 3e19 and 5e-20 across quads (the world the GPU test renders) (neither wherever the
    restatement meets a subnormal or non-finite value, both elsewhere); material slots inside, unset, beyond the instance's table and beyond 63

The program itself checks that the blob, its offsets, the pair section and hot_bytes() are what they were without the section, and that a
scene beyond the staging limit gets none."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
F32, U32 = np.float32, np.uint32
TREE_REFERENCE, TREE_SAH, TREE_DEVICE = 0, 1, 2
NORMAL_VALID, MAPPED_VALID = 1, 2
LEAF, COUNT_MASK, HAS_NORMALS, MATERIAL_MASK = 0x80000000, 0x1FFFFFFF, 0x80000000, 0x00FFFFFF


# ---- the worlds of tests/pair_records_main.cpp, as arrays ----
def _mix(v):
    v &= 0xFFFFFFFF
    v ^= v >> 16
    v = (v * 0x7FEB352D) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 0x846CA68B) & 0xFFFFFFFF
    return v ^ (v >> 16)


def _coordinate(k):
    return F32(_mix(k) >> 8) * F32(8.0 / 16777216.0) - F32(4.0)


def _normalized(v):
    return v * (F32(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def pair_world(meshes, instance_mesh, split_world, seed):
    """`meshes`: per mesh the triangle counts of its leaves (one: the root is a leaf; two: an inner root over two leaves)"""
    from rayzath_amd import _abi
    from rayzath_amd.scene import FlatScene

    def leaf(begin, count):
        n = np.zeros(1, _abi.node_dtype)[0]
        n["bb_min"], n["bb_max"], n["begin"], n["meta"] = -4.0, 4.0, begin, LEAF | count
        return n

    def inner(first_child):
        n = leaf(first_child, 0)
        n["meta"] = 2 << 29
        return n

    n_inst = len(instance_mesh)
    nodes = [inner(1), leaf(0, n_inst // 2), leaf(n_inst // 2, n_inst - n_inst // 2)] if split_world else [leaf(0, n_inst)]
    tris, attrs, roots = [], [], []
    for leaves in meshes:
        roots.append(len(nodes))
        if len(leaves) == 1:
            nodes.append(leaf(len(tris), leaves[0]))
        else:
            nodes += [inner(len(nodes) + 1), leaf(len(tris), leaves[0]), leaf(len(tris) + leaves[0], leaves[1])]
        for t in range(sum(leaves)):
            tri, attr = np.zeros(1, _abi.tri_dtype)[0], np.zeros(1, _abi.tri_attr_dtype)[0]
            k = seed * 0x10001 + len(tris) * 16
            v1, v2, v3 = (np.array([_coordinate(k + 3 * c + a) for a in range(3)], F32) for c in range(3))
            tri["v1"], tri["v2"], tri["v3"], tri["source_index"] = v1, v2, v3, t
            attr["face_normal"] = _normalized(np.cross(v2 - v3, v2 - v1).astype(F32))
            tris.append(tri), attrs.append(attr)
    instances = np.zeros(n_inst, _abi.instance_dtype)
    for i in range(n_inst):
        r = instances[i]
        r["blas_root"], r["scale"], r["position"] = roots[instance_mesh[i]], 1.0 + 0.25 * i, float(i)
        r["bb_min"], r["bb_max"] = -40.0, 40.0
        r["x_axis"], r["y_axis"], r["z_axis"] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
        r["material_base"], r["material_count"] = i, 1
    materials = np.zeros(2, _abi.material_dtype)
    for f in ("texture", "normal_map", "metalness_map", "roughness_map", "emission_map"):
        materials[f] = -1
    return FlatScene(nodes=np.array(nodes, _abi.node_dtype), tlas_root=0, tlas_order=np.arange(n_inst, dtype=U32),
                     tris=np.array(tris, _abi.tri_dtype) if tris else np.zeros(0, _abi.tri_dtype),
                     tri_attrs=np.array(attrs, _abi.tri_attr_dtype) if attrs else np.zeros(0, _abi.tri_attr_dtype),
                     instances=instances, inst_materials=np.ones(n_inst, np.int32), materials=materials, textures=np.zeros(0, _abi.texture_dtype),
                     texels=np.zeros(0, np.uint8), spot_lights=np.zeros(0, _abi.spot_light_dtype), direct_lights=np.zeros(0, _abi.direct_light_dtype))


PAIR_WORLDS = [  # name, meshes, instance -> mesh, split world, tree mode (tests/pair_records_main.cpp: main)
    ("small leaves", [[1], [2], [3], [4], [5], [8], [9]], [0, 1, 2, 3, 4, 5, 6, 0], False, TREE_REFERENCE),
    ("large leaves", [[12], [31], [32]], [1, 0, 2, 1], False, TREE_REFERENCE),
    ("inner root beside leaves", [[3], [3, 2], [5]], [0, 1, 2, 1], False, TREE_REFERENCE),
    ("empty leaf", [[0], [2]], [0, 1], False, TREE_REFERENCE),
    ("three instances", [[4]], [0, 0, 0], False, TREE_REFERENCE),
    ("nine instances", [[2]], [0] * 9, False, TREE_REFERENCE),
    ("split world", [[2], [3]], [0, 1, 0, 1], True, TREE_REFERENCE),
    ("inner roots only", [[2, 2]], [0, 0], False, TREE_REFERENCE),
    ("device trees", [[12], [3]], [0, 1], False, TREE_DEVICE),
    ("surface-area trees", [[12], [3]], [0, 1], False, TREE_SAH),
]


# ---- the restatement ----
class Seen:
    """float32 values pass through see(): `bad` marks the triangles for which one of them was subnormal, infinite or NaN"""

    def __init__(self, n):
        self.bad = np.zeros(n, bool)

    @staticmethod
    def wrong(x):
        return ~np.isfinite(x) | ((x != 0) & (np.abs(x) < np.finfo(F32).tiny))

    def see(self, x):   # one row per triangle
        assert x.dtype == F32 and x.shape[0] == len(self.bad)
        self.bad |= self.wrong(x).reshape(len(self.bad), -1).any(1)
        return x

    def see_placement(self, x):   # of the instance: every triangle's concern
        assert x.dtype == F32
        self.bad |= bool(self.wrong(x).any())

    def forward(self, axes, v):   # (xa * v.x + ya * v.y) + za * v.z
        xa, ya, za = axes
        see = self.see
        return see(see(see(xa[None, :] * v[:, 0:1]) + see(ya[None, :] * v[:, 1:2])) + see(za[None, :] * v[:, 2:3]))

    def normalized(self, v):   # v * (1 / sqrt((x x + y y) + z z))
        see = self.see
        xx, yy, zz = see(v[:, 0] * v[:, 0]), see(v[:, 1] * v[:, 1]), see(v[:, 2] * v[:, 2])
        r = see(F32(1.0) / see(np.sqrt(see(see(xx + yy) + zz))))
        return see(v * r[:, None])


def mesh_range(flat, root):
    lo, hi, todo = 0xFFFFFFFF, 0, [int(root)]
    while todo:
        n = flat.nodes[todo.pop()]
        if int(n["meta"]) & LEAF:
            count = int(n["meta"]) & COUNT_MASK
            if count:
                lo, hi = min(lo, int(n["begin"])), max(hi, int(n["begin"]) + count)
        else:
            todo += [int(n["begin"]), int(n["begin"]) + 1]
    return lo, hi


def restate(flat):
    """the section of `flat` under the snapshot's own trees: (table, records[pair, side, 8 words])"""
    n_inst = len(flat.instances)
    table, records = np.zeros((n_inst + 3) & ~3, U32), []
    with np.errstate(all="ignore"):
        for i in sorted(set(int(k) for k in flat.tlas_order)):
            inst = flat.instances[i]
            lo, hi = mesh_range(flat, inst["blas_root"])
            if lo >= hi:
                continue
            table[i] = (len(records) - lo) & 0xFFFFFFFF
            n = hi - lo
            scale = inst["scale"].astype(F32)
            axes = (inst["x_axis"].astype(F32), inst["y_axis"].astype(F32), inst["z_axis"].astype(F32))
            fn = flat.tri_attrs["face_normal"][lo:hi].astype(F32)
            flags = flat.tris["material_flags"][lo:hi].astype(np.int64)
            slot = np.minimum(flags & MATERIAL_MASK, 63)
            base, count = int(inst["material_base"]), int(inst["material_count"])
            mat = np.array([int(flat.inst_materials[base + s]) if s < count else -1 for s in slot], np.int64)
            surface = np.where(mat < 0, 1, mat).astype(U32)
            rec = np.zeros((n, 2, 8), U32)
            for side in (0, 1):
                ef = F32(side) * F32(2.0) - F32(1.0)
                s = Seen(n)
                for v in (scale, *axes):
                    s.see_placement(v)
                s.see(fn)
                normal = s.normalized(s.forward(axes, s.see(s.see(fn * ef) / scale[None, :])))
                mapped = s.see(s.normalized(s.forward(axes, s.see(fn / scale[None, :]))) * ef)
                valid = np.where(s.bad, 0, NORMAL_VALID | np.where(flags & HAS_NORMALS, 0, MAPPED_VALID)).astype(U32)
                rec[:, side, 0:3], rec[:, side, 4:7] = normal.view(U32), mapped.view(U32)
                rec[:, side, 3], rec[:, side, 7] = surface, valid
            records += list(rec)
    return table, np.array(records, U32).reshape(-1, 2, 8)


SCENES = ("cornell", "placements", "vertex_normals", "extreme_cubes", "extremes", "material_slots")   # of tests/surface_scenes.py


# ---- the child process ----
def _write_scene(f, flat, tree_mode):
    f.write(struct.pack("<9I", tree_mode, len(flat.nodes), flat.tlas_root, len(flat.tlas_order), len(flat.tris), len(flat.instances),
                        len(flat.inst_materials), len(flat.materials), 0))
    for a in (flat.nodes, flat.tlas_order, flat.tris, flat.tri_attrs, flat.instances, flat.inst_materials, flat.materials):
        f.write(np.ascontiguousarray(a).tobytes())


@pytest.fixture(scope="module")
def sections(built, tmp_path_factory):
    """name -> (flat, tree mode, own_trees, section bytes) for every scene, from ONE run of the program"""
    import surface_scenes
    from rayzath_amd.scene import flatten
    tmp = tmp_path_factory.mktemp("surface_records")
    cases = [(name, pair_world(meshes, inst, split, k + 1), mode) for k, (name, meshes, inst, split, mode) in enumerate(PAIR_WORLDS)]
    for name in SCENES:
        cases.append((name, flatten(getattr(surface_scenes, name)()), TREE_REFERENCE))
    exe, fin, fout = str(tmp / "surface_records"), str(tmp / "in.bin"), str(tmp / "out.bin")
    subprocess.run(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "hiprz_scene_host.cpp"),
                    os.path.join(CSRC, "hiprz_host.cpp"), os.path.join(ROOT, "tests", "surface_records_main.cpp"), "-o", exe], check=True)
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, flat, mode in cases:
            _write_scene(f, flat, mode)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and f"surface records: {len(cases)} scenes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    out, data, at = {}, open(fout, "rb").read(), 0
    for name, flat, mode in cases:
        own_trees, _, _, n = struct.unpack_from("<4I", data, at)
        out[name] = (flat, mode, own_trees, data[at + 16:at + 16 + n])
        at += 16 + n
    assert at == len(data)
    return out


def _split(flat, section):
    words = np.frombuffer(section, U32)
    n_table = (len(flat.instances) + 3) & ~3
    return words[:n_table], words[n_table:].reshape(-1, 2, 8)


ALL = [w[0] for w in PAIR_WORLDS] + list(SCENES)


@pytest.mark.parametrize("name", ALL)
def test_section_equals_the_restatement(sections, name):
    flat, mode, own_trees, section = sections[name]
    if mode != TREE_REFERENCE:
        assert own_trees and section == b"", f"{name}: trees rebuilt at upload are never staged and have no section"
        return
    assert not own_trees
    table, records = _split(flat, section)
    want_table, want_records = restate(flat)
    assert np.array_equal(table, want_table), name
    assert records.shape == want_records.shape, name
    differ = np.argwhere(records != want_records)
    assert len(differ) == 0, f"{name}: first difference at (pair, side, word) {differ[0]}: {records[tuple(differ[0])]:#x} != {want_records[tuple(differ[0])]:#x}"
    # every hit a walk can report finds its own instance's record of its triangle
    for i in set(int(k) for k in flat.tlas_order):
        lo, hi = mesh_range(flat, flat.instances[i]["blas_root"])
        pairs = (int(table[i]) + np.arange(lo, max(hi, lo), dtype=np.int64)) & 0xFFFFFFFF
        assert (pairs < len(records)).all(), (name, i)


def test_config_b_has_72_valid_records_and_sides_that_are_not_negations(sections):
    flat, _, _, section = sections["cornell"]
    assert len(flat.instances) == 8 and len(flat.tris) == 16
    _, records = _split(flat, section)
    assert records.shape == (36, 2, 8) and (records[:, :, 7] == (NORMAL_VALID | MAPPED_VALID)).all()
    inside, outside = records[:, 0, 0:3], records[:, 1, 0:3]
    zero = (inside & 0x7FFFFFFF) == 0
    assert np.array_equal(zero, (outside & 0x7FFFFFFF) == 0)
    assert np.array_equal(inside[~zero] ^ 0x80000000, outside[~zero]), "the non-zero components are each other's negation"
    assert (inside[zero] == outside[zero]).any(), "somewhere a zero has the SAME sign on both sides of a wall: one record cannot serve both"


def _of_instance(flat, table, records, i):
    """the record pairs of instance i's triangles, and the triangle range"""
    lo, hi = mesh_range(flat, flat.instances[i]["blas_root"])
    first = (int(table[i]) + lo) & 0xFFFFFFFF
    return records[first:first + hi - lo], lo, hi


def test_flags_of_the_special_scenes(sections):
    flat, _, _, section = sections["vertex_normals"]
    table, records = _split(flat, section)
    smooth = [i for i in range(len(flat.instances)) if _of_instance(flat, table, records, i)[0].shape[0] == 48]
    assert len(smooth) == 2
    for i in smooth:
        rec, lo, hi = _of_instance(flat, table, records, i)
        assert (flat.tris["material_flags"][lo:hi] & HAS_NORMALS).all()
        assert (rec[:, :, 7] == NORMAL_VALID).all(), "vertex normals: the normal is valid, the mapped normal is interpolated per hit"

    flat, _, _, section = sections["extreme_cubes"]
    table, records = _split(flat, section)
    degenerate, big, small, plain = 2, 3, 4, 5   # instance ids (surface_scenes.extreme_cubes: floor and lamp come first)
    valid = lambda i: _of_instance(flat, table, records, i)[0][:, :, 7]
    flagged = valid(degenerate)
    assert sorted(flagged.tolist()) == [[0, 0], [3, 3], [3, 3]], "only the zero-area triangle is flagged"
    for i in (big, small):
        v = valid(i)
        assert set(v.ravel().tolist()) == {0, 3} and (v[:, 0] == v[:, 1]).all(), f"instance {i}: the faces across the scaled axis are flagged, the others are not"
    assert (valid(plain) == 3).all()

    flat, _, _, section = sections["extremes"]   # the scene the GPU test renders: both scaled quads flagged as a whole
    table, records = _split(flat, section)
    valid = lambda i: _of_instance(flat, table, records, i)[0][:, :, 7]
    assert sorted(valid(degenerate).tolist()) == [[0, 0], [3, 3], [3, 3]]
    assert (valid(big) == 0).all() and (valid(small) == 0).all() and (valid(plain) == 3).all() and (valid(0) == 3).all() and (valid(1) == 3).all()

    flat, _, _, section = sections["material_slots"]
    table, records = _split(flat, section)
    four, one = 2, 3
    rec, lo, hi = _of_instance(flat, table, records, four)
    slots = np.array([0, 0, 1, 1, 2, 2, 3, 3, 9, 9, 70, 200])[flat.tris["source_index"][lo:hi]]
    mats = flat.inst_materials[int(flat.instances[four]["material_base"]):][:4]
    assert mats[2] == -1
    want = np.array([int(mats[s]) if s < 4 and mats[s] >= 0 else 1 for s in slots])
    assert np.array_equal(rec[:, 0, 3], want) and np.array_equal(rec[:, 1, 3], want)
    rec, _, _ = _of_instance(flat, table, records, one)
    only = int(flat.inst_materials[int(flat.instances[one]["material_base"])])
    assert np.array_equal(rec[:, 0, 3], np.where(slots == 0, only, 1))
