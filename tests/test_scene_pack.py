"""rayzath_amd/csrc/hiprz_scene_host.cpp — the pure-host half of scene mirroring — run WITHOUT a GPU: the unit, hiprz_host.cpp and the
shim tests/scene_pack_shim.cpp are compiled with g++ under UBSan and libstdc++'s assertions, and every host stage of an upload (check,
choose trees, derive, pack, shadow tree) runs over the 60 generated scenes of tests/generated_scenes.py (the empty world, mirrored and
strongly non-uniform scales, one-leaf meshes, degenerate triangles) — and, for the unit-scale flag of the packed instance record, over
variants of them in which instances get scale (1, 1, 1) or exactly one or two components equal to 1 (no generated scene has either).
What the stages produce is compared, bit for bit, with a numpy restatement of the device layout hiprz_device.hpp reads: the hot blob's
sections, the relayouted nodes with interleaved boxes, the packed instance record, the edge form of the triangles, the 64-byte walk records, the shadow rays' own world tree.

The checks run in a child process (this file as a script): a sanitizer or assertion abort fails one test, not the session."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
END = 0xFFFFFFFF
TREE_REFERENCE, TREE_SAH, TREE_DEVICE = 0, 1, 2
LDS_LIMIT = 52 * 1024
PARTIAL = [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)]


class View(C.Structure):   # rzp_view of tests/scene_pack_shim.cpp
    _fields_ = [("blob", C.c_void_p), ("blob_bytes", C.c_uint64), ("off", C.c_uint32 * 7),
                ("tree", C.c_uint32), ("own_trees", C.c_uint32), ("identity_order", C.c_uint32), ("fast_div", C.c_uint32),
                ("tlas_root", C.c_uint32), ("node_capacity", C.c_uint32), ("world_region", C.c_uint32), ("n_device_meshes", C.c_uint32),
                ("scene", C.c_void_p), ("reachable", C.c_void_p), ("new_index", C.c_void_p), ("nodes", C.c_void_p), ("n_nodes", C.c_uint32),
                ("skip", C.c_void_p), ("nodes64", C.c_void_p), ("instances", C.c_void_p), ("boxes", C.c_void_p), ("members", C.c_void_p),
                ("n_members", C.c_uint32), ("shadow_records", C.c_void_p), ("n_shadow_records", C.c_uint32), ("shadow_order", C.c_void_p),
                ("device_meshes", C.c_void_p), ("instance_mesh", C.c_void_p)]


mesh_dtype = np.dtype([("tri_first", "<u4"), ("n_tris", "<u4"), ("ref_first", "<u4"), ("region", "<u4"), ("leaf_slot", "<u4"), ("n_slots", "<u4"),
                       ("bb_min", "<f4", 3), ("bb_max", "<f4", 3)])   # hiprz::DeviceMesh


def _array(address, dtype, count):
    """a copy of `count` records at `address`"""
    dtype = np.dtype(dtype)
    if not count:
        return np.zeros(0, dtype)
    return np.frombuffer(C.string_at(address, count * dtype.itemsize), dtype=dtype).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pad16(n):
    return (n + 15) & ~15


class Pack:
    """one upload's host stages over `flat` under `tree_mode`"""

    def __init__(self, lib, flat, tree_mode):
        from rayzath_amd import _abi
        self.view, msg = View(), C.create_string_buffer(256)
        self.handle = lib.rzp_pack(C.byref(flat.struct), tree_mode, LDS_LIMIT, C.byref(self.view), msg, 256)
        assert self.handle, msg.value
        v = self.view
        self.blob = _array(v.blob, np.uint8, v.blob_bytes)
        self.off = list(v.off)
        sc = _abi.Scene.from_address(v.scene)
        self.scene_nodes = _array(sc.nodes, _abi.node_dtype, sc.n_nodes)           # of the snapshot that was packed
        self.scene_instances = _array(sc.instances, _abi.instance_dtype, sc.n_instances)
        self.scene_tris = _array(sc.tris, _abi.tri_dtype, sc.n_tris)
        self.scene_attrs = _array(sc.tri_attrs, _abi.tri_attr_dtype, sc.n_tris)
        self.reachable = _array(v.reachable, np.uint8, max(sc.n_nodes, 1))[:sc.n_nodes].astype(bool)
        self.new_index = _array(v.new_index, np.uint32, sc.n_nodes)
        self.nodes = _array(v.nodes, _abi.node_dtype, v.n_nodes)
        self.skip = _array(v.skip, np.uint32, max(v.node_capacity, 1))
        self.nodes64 = _array(v.nodes64, np.uint32, max(v.node_capacity, 1) * 16).reshape(-1, 16)
        self.instances = _array(v.instances, _abi.instance_dtype, sc.n_instances)
        self.boxes = _array(v.boxes, np.float32, sc.n_instances * 6).reshape(-1, 2, 3)
        self.members = _array(v.members, np.uint32, v.n_members)
        self.shadow_records = _array(v.shadow_records, np.uint32, v.n_shadow_records * 16).reshape(-1, 16)
        self.shadow_order = _array(v.shadow_order, np.uint32, v.n_members if v.n_shadow_records else 0)
        self.device_meshes = _array(v.device_meshes, mesh_dtype, v.n_device_meshes)
        self.instance_mesh = _array(v.instance_mesh, np.uint32, sc.n_instances)
        self.tlas_root_in, self.n_tlas_order = sc.tlas_root, sc.n_tlas_order
        self.tlas_order = _array(sc.tlas_order, np.uint32, sc.n_tlas_order)
        n_slots = np.where(self.device_meshes["region"] != END, 2 * self.device_meshes["n_tris"] - 1, 0).astype(np.uint32)
        self.entered_roots = np.zeros(sc.n_instances, np.uint32)
        self.emitted = lib.rzp_enter_device_roots(self.handle, n_slots.ctypes.data, 7, self.entered_roots.ctypes.data)
        self.pretended_slots = n_slots
        lib.rzp_free(self.handle)

    def section(self, k, dtype, count):
        dtype = np.dtype(dtype)
        return self.blob[self.off[k]:self.off[k] + count * dtype.itemsize].view(dtype)


def _check_sections(p, flat):
    """16-byte aligned sections in the order nodes, tlas_order, instances, tris, attrs, materials, inst_materials; hot_bytes is the total"""
    sizes = [32 * len(p.nodes), 4 * len(flat.tlas_order), 112 * len(flat.instances), 48 * len(flat.tris), 96 * len(flat.tris),
             48 * len(flat.materials), 4 * len(flat.inst_materials)]
    assert p.off[0] == 0 and all(o % 16 == 0 for o in p.off)
    for k in range(6):
        assert p.off[k + 1] == p.off[k] + _pad16(sizes[k]), k
    assert len(p.blob) == p.off[6] + _pad16(sizes[6])
    assert np.array_equal(p.section(1, np.uint32, len(flat.tlas_order)), flat.tlas_order)
    assert p.section(5, np.uint8, sizes[5]).tobytes() == flat.materials.tobytes()
    assert p.section(6, np.uint8, sizes[6]).tobytes() == flat.inst_materials.tobytes()
    assert p.section(0, np.uint8, sizes[0]).tobytes() == p.nodes.tobytes()
    assert p.section(2, np.uint8, sizes[2]).tobytes() == p.instances.tobytes()


def _check_nodes(p):
    """record new_index[i] is input node i: the box interleaved (min.x, max.x, min.y, max.y, min.z, max.z), a leaf's range kept, an inner
    node's children remapped and adjacent; each 64-byte walk record is its node + eight octant links, octant 0 = the reference order's"""
    src, idx = p.scene_nodes, p.new_index.astype(np.int64)
    assert len(set(idx.tolist())) == len(idx) and (idx < len(p.nodes)).all()
    rec = p.nodes[idx]
    box = np.concatenate([_bits(rec["bb_min"]), _bits(rec["bb_max"])], axis=1).reshape(-1, 6)
    assert np.array_equal(box[:, 0::2], _bits(src["bb_min"]).reshape(-1, 3)) and np.array_equal(box[:, 1::2], _bits(src["bb_max"]).reshape(-1, 3))
    assert np.array_equal(rec["meta"], src["meta"])
    leaf = (src["meta"] & 0x80000000) != 0
    assert np.array_equal(rec["begin"][leaf], src["begin"][leaf])
    first = src["begin"][~leaf].astype(np.int64)
    assert np.array_equal(rec["begin"][~leaf], idx[first]) and np.array_equal(idx[first + 1], idx[first] + 1)
    n = len(p.nodes)
    assert p.nodes64[:n, :8].tobytes() == p.nodes.tobytes()
    links = p.nodes64[:n, 8:]
    assert ((links == END) | (links < n)).all()
    reached = idx[p.reachable]
    assert np.array_equal(links[reached, 0], p.skip[reached])
    # all eight octants, restated: under octant o an inner node of partition type t is left towards its SECOND child first when bit t of
    # o is set (type 3 reads bit 3 = 0); the child visited first links to its sibling, the other inherits the parent's link; roots end
    want = np.full((n, 8), END, np.uint32)
    meta, begin = p.nodes["meta"], p.nodes["begin"]
    for k in range(n):                                   # parents precede their children in the relayout
        if not (meta[k] & 0x80000000) and begin[k] > k:
            c0, t = int(begin[k]), int(meta[k] >> 29) & 3
            for o in range(8):
                flip = (o >> t) & 1
                want[c0 + flip, o] = c0 + 1 - flip
                want[c0 + 1 - flip, o] = want[k, o]
    assert np.array_equal(links[reached], want[reached])
    # ... and an independent walk per octant over the records themselves: it enters every node of its tree once and ends
    roots = ([int(idx[p.tlas_root_in])] if len(p.scene_instances) else []) + sorted(set(idx[p.scene_instances["blas_root"][p.tlas_order]].tolist()))
    for root in roots:
        size, stack = 0, [root]
        while stack:
            k = stack.pop()
            size += 1
            if not (meta[k] & 0x80000000):
                stack += [int(begin[k]), int(begin[k]) + 1]
        for o in range(8):
            seen, k = set(), root
            while k != END:
                assert k not in seen and len(seen) < size, (root, o)
                seen.add(k)
                k = int(begin[k]) + ((o >> (int(meta[k] >> 29) & 3)) & 1) if not (meta[k] & 0x80000000) else int(links[k, o])
            assert len(seen) == size, (root, o)


def _check_box_layout(lib, p):
    """interleave_box and deinterleave_box, the one definition of each: the packer's records come from the first, hiprz_download_trees and
    hiprz_rebuild_trees read them back through the second"""
    src = p.scene_nodes.copy()
    lib.rzp_interleave(src.ctypes.data, len(src))
    lo, hi = _bits(p.scene_nodes["bb_min"]).reshape(-1, 3), _bits(p.scene_nodes["bb_max"]).reshape(-1, 3)
    assert np.array_equal(_bits(src["bb_min"]).reshape(-1, 3), np.stack([lo[:, 0], hi[:, 0], lo[:, 1]], axis=1))
    assert np.array_equal(_bits(src["bb_max"]).reshape(-1, 3), np.stack([hi[:, 1], lo[:, 2], hi[:, 2]], axis=1))
    back = p.nodes.copy()
    lib.rzp_deinterleave(back.ctypes.data, len(back))
    back = back[p.new_index.astype(np.int64)]
    assert np.array_equal(_bits(back["bb_min"]), _bits(p.scene_nodes["bb_min"])) and np.array_equal(_bits(back["bb_max"]), _bits(p.scene_nodes["bb_max"]))


def _check_device_plan(p, flat):
    """HIPRZ_TREE_DEVICE: one placeholder leaf per mesh; behind the uploaded prefix the world tree's region (2 * instances + 1 slots), then
    per mesh of more than 4 triangles a region of 2 n - 1 slots — every region at an odd slot, none overlapping, all inside node_capacity;
    after a build the instances enter at the regions' first slots"""
    v, m = p.view, p.device_meshes
    assert v.world_region % 2 == 1 and v.world_region >= len(p.nodes)
    cursor = v.world_region + 2 * len(flat.instances) + 1
    ranges = sorted((int(a), int(a) + int(c)) for a, c in zip(m["tri_first"], m["n_tris"]))
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and (not ranges or (ranges[0][0] == 0 and ranges[-1][1] == len(flat.tris)))
    for k in range(len(m)):
        assert (m["region"][k] == END) == (m["n_tris"][k] <= 4), k
        if m["region"][k] != END:
            assert m["region"][k] % 2 == 1 and m["region"][k] >= cursor, k
            cursor = int(m["region"][k]) + 2 * int(m["n_tris"][k]) - 1
    assert v.node_capacity == cursor and len(p.skip) == cursor and len(p.nodes64) == cursor
    used = p.instance_mesh != END
    assert used.all() and np.array_equal(m["leaf_slot"][p.instance_mesh], p.instances["blas_root"])
    region = m["region"][p.instance_mesh]
    assert np.array_equal(p.entered_roots, np.where(region != END, region, p.instances["blas_root"]))
    assert p.emitted == 7 + int(p.pretended_slots.sum())


def _check_instances(p):
    """the packed record: pad0 flags a unit scale, the box interleaved with max.y parked in pad2 — and read back through the accessor"""
    src, got = p.scene_instances, p.instances
    assert np.array_equal(_bits(p.boxes[:, 0]), _bits(src["bb_min"]).reshape(-1, 3)) and np.array_equal(_bits(p.boxes[:, 1]), _bits(src["bb_max"]).reshape(-1, 3))
    lo, hi = _bits(src["bb_min"]).reshape(-1, 3), _bits(src["bb_max"]).reshape(-1, 3)
    assert np.array_equal(_bits(got["bb_min"]).reshape(-1, 3), np.stack([lo[:, 0], hi[:, 0], lo[:, 1]], axis=1))
    assert np.array_equal(got["pad2"], hi[:, 1])
    assert np.array_equal(_bits(got["bb_max"]).reshape(-1, 3), np.stack([lo[:, 2], hi[:, 2], np.zeros(len(src), np.uint32)], axis=1))
    assert np.array_equal(got["pad0"], (src["scale"] == np.float32(1.0)).all(-1).astype(np.uint32))
    assert np.array_equal(got["blas_root"], p.new_index[src["blas_root"]])
    for field in ("position", "scale", "x_axis", "y_axis", "z_axis", "material_base", "material_count", "pad1", "pad3"):
        assert np.array_equal(_bits(got[field]), _bits(src[field])), field


def _check_triangles(p, flat, refpos):
    """device triangle i derives from input triangle refpos[i]: v1 kept, the edges v2 - v1 and v3 - v1 in float32, v2 and v3 bit for bit
    in the attribute record's padding, pad0 = refpos[i]"""
    from rayzath_amd import _abi
    n = len(flat.tris)
    tris, attrs = p.section(3, _abi.tri_dtype, n), p.section(4, _abi.tri_attr_dtype, n)
    src, src_attrs = flat.tris[refpos], flat.tri_attrs[refpos]
    assert np.array_equal(tris["pad0"], refpos)
    assert np.array_equal(_bits(tris["v1"]), _bits(src["v1"]))
    assert np.array_equal(_bits(tris["v2"]), _bits(src["v2"] - src["v1"])) and np.array_equal(_bits(tris["v3"]), _bits(src["v3"] - src["v1"]))
    assert np.array_equal(tris["material_flags"], src["material_flags"]) and np.array_equal(tris["source_index"], src["source_index"])
    parked = np.stack([attrs["pad0"], attrs["pad1"], attrs["pad2"], attrs["pad3"], attrs["pad4"][:, 0], attrs["pad4"][:, 1]], axis=1) if n else np.zeros((0, 6), np.float32)
    assert np.array_equal(_bits(parked).reshape(-1, 6), np.concatenate([_bits(src["v2"]).reshape(-1, 3), _bits(src["v3"]).reshape(-1, 3)], axis=1))
    for field in ("n1", "n2", "n3", "face_normal", "t1", "t2", "t3"):
        assert np.array_equal(_bits(attrs[field]), _bits(src_attrs[field])), field


def _check_shadow_tree(p):
    """binary, one instance per leaf, `order` a permutation of the members, a leaf's 24 box bytes the packed instance's, and the walk
    inner -> first child / leaf -> link from record 0 visits every record once and ends"""
    m, rec = len(p.members), p.shadow_records
    assert len(rec) == 2 * m and sorted(p.shadow_order.tolist()) == p.members.tolist()
    visited, n, leaves = [], 0, 0
    while n != END:
        assert n < 2 * m - 1 and len(visited) < 2 * m, "the walk leaves the tree or does not end"
        visited.append(n)
        r = rec[n]
        assert (r[8:] == r[8]).all()
        if r[7] & 0x80000000:
            assert r[7] == 0x80000001 and r[6] < m
            inst = p.instances[p.shadow_order[r[6]]]
            assert r[:6].tobytes() == inst["bb_min"].tobytes() + inst["pad2"].tobytes() + inst["bb_max"][:2].tobytes()
            leaves, n = leaves + 1, int(r[8])
        else:
            assert (r[7] & 0x1FFFFFFF) == 0 and r[6] + 1 < 2 * m - 1
            assert rec[r[6]][8] == r[6] + 1 and rec[r[6] + 1][8] == r[8]      # first child -> its sibling -> whatever follows the parent
            n = int(r[6])
    assert sorted(visited) == list(range(2 * m - 1)) and leaves == m


def _child(so_path, mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import generated_scenes
    lib = C.CDLL(so_path)
    lib.rzp_pack.restype, lib.rzp_pack.argtypes = C.c_void_p, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]
    lib.rzp_free.argtypes = [C.c_void_p]
    lib.rzp_interleave.argtypes = lib.rzp_deinterleave.argtypes = [C.c_void_p, C.c_uint32]
    lib.rzp_enter_device_roots.restype, lib.rzp_enter_device_roots.argtypes = C.c_uint32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    done = 0
    for seed in generated_scenes.SEEDS:
        flat = generated_scenes.flat_scene(seed)[0]
        if mode == "scales":   # the unit-scale flag: all three components exactly 1, nothing less
            if not len(flat.instances):
                continue
            from rayzath_amd.scene import FlatScene
            for variant in ("unit", "partial"):
                inst = flat.instances.copy()
                for i in range(len(inst)):
                    if variant == "unit" and i % 2 == 0:
                        inst["scale"][i] = 1.0
                    elif variant == "partial":
                        mask = PARTIAL[(seed + i) % len(PARTIAL)]
                        inst["scale"][i] = np.where(mask, np.float32(1.0), inst["scale"][i])
                changed = FlatScene(**{**flat.to_npz_dict(), "instances": inst})
                p = Pack(lib, changed, TREE_REFERENCE)
                _check_instances(p)
                flags = p.instances["pad0"]
                assert flags[0::2].all() and not flags[1::2].any() if variant == "unit" else not flags.any()
            done += 1
            continue
        if mode in ("reference", "shadow"):
            p = Pack(lib, flat, TREE_REFERENCE)
            assert not p.view.own_trees and p.view.tree == TREE_REFERENCE and p.view.node_capacity == len(p.nodes)
            if mode == "shadow":
                if len(p.members):
                    _check_shadow_tree(p)
                    done += 1
                continue
            _check_sections(p, flat)
            _check_nodes(p)
            _check_box_layout(lib, p)
            _check_instances(p)
            _check_triangles(p, flat, np.arange(len(flat.tris), dtype=np.uint32))
        else:   # the placeholder trees: the snapshot is rewritten, triangles may move
            from rayzath_amd import _abi
            p = Pack(lib, flat, TREE_SAH if mode == "sah" else TREE_DEVICE)
            assert bool(p.view.own_trees) == (len(flat.tris) != 0)
            refpos = p.section(3, _abi.tri_dtype, len(flat.tris))["pad0"].copy()
            assert sorted(refpos.tolist()) == list(range(len(flat.tris)))
            _check_sections(p, flat)
            _check_nodes(p)
            _check_instances(p)
            _check_triangles(p, flat, refpos)
            if mode == "device" and p.view.own_trees:
                _check_device_plan(p, flat)
        done += 1
    print(f"{mode}: {done} scenes ok")


@pytest.fixture(scope="module")
def shim(built, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scene_pack") / "libscene_pack.so")
    subprocess.run(["g++", *FLAGS, "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "hiprz_scene_host.cpp"),
                    os.path.join(CSRC, "hiprz_host.cpp"), os.path.join(ROOT, "tests", "scene_pack_shim.cpp"), "-o", so], check=True)
    return so


@pytest.mark.parametrize("mode,scenes", [("reference", 60), ("sah", 60), ("device", 60), ("shadow", 57), ("scales", 57)])
def test_host_stages_of_an_upload_over_the_generated_scenes(shim, mode, scenes):
    """reference: the layout checks with the snapshot's trees; sah / device: sanitizer-clean with rewritten snapshots, pad0 a permutation,
    triangle i derived from input triangle pad0[i], device also the plan of the regions; shadow: the shadow rays' tree of every scene with a
    world member (3 of the 60 are empty); scales: the packed instance records of the unit-scale variants of every scene with an instance."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), shim, mode], capture_output=True, text=True)
    assert r.returncode == 0 and f"{mode}: {scenes} scenes ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
