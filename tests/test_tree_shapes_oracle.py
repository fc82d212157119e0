"""The scenes of tests/tree_shape_scenes.py, proven on the CPU: every scene holds the tree shape it is named for under both host builders
(libhiprz.so's and the oracle's), the validator accepts it, the oracle's frames are finite, the camera sees the mesh and the shadow rays
test its triangles; and the comparison has teeth on exactly these shapes: four mutant oracles (oracle/Makefile), each with one bug of a
walk in a leaf that does not fit its step or at a Size node, standing in for the device, break the lockstep rule that
tests/test_tree_shapes_gpu.py holds the kernels to on at least one scene of the module — and on none of the 60 generated scenes of the
older sweep (generated_scenes.SEEDS), whose reference trees have no Size node, no leaf above 8 below a mesh's root and no leaf above 64
at all.  Run with -s for the tables.

The mutants, as built: `leaf_eight` leaves the root leaf of a one-leaf mesh alone (the generated scenes' cubes and 18-triangle soups are
root leaves of 12 and 18, walked by code of their own); it is the walk of a leaf BELOW the root that stops after 8.  `tie_later` meets
the generated scenes' duplicate triangles 16 positions apart in one root leaf, but a duplicate there carries its original's material
and attributes: the later winner changes no compared value.  `shadow_sixtyfour` also acts in the compat modes' shadow walk."""
import ctypes as C

import numpy as np
import pytest

import generated_scenes as G
import lockstep
import oracle
import tree_shape_scenes as T
from lockstep import OracleDevice, bad
from rayzath_amd import _abi
from rayzath_amd.scene import HostBackend, flatten

THREADS = 4   # of the oracle's; its frames do not depend on the count
# mutant -> scenes that must flag it: the shape the bug needs (any other scene may flag it too)
MUTANTS = {
    "leaf_eight": ("big_leaf_9", "big_leaf_13_sky", "big_leaf_257"),
    "size_second": ("big_leaf_9_sky", "size_chain", "size_chain_sky"),
    "tie_later": ("ties_across_chunks", "ties_across_chunks_sky"),
    "shadow_sixtyfour": ("big_leaf_65", "big_leaf_257", "root_leaf_300"),
}


def _base(name):
    return name[:-4] if name.endswith("_sky") else name


def _renderer(scene, lib=None, mode=0):
    flat, cam, cfg = lockstep.flat_scene(scene)[:3]
    return oracle.OracleRenderer(flat, cam, cfg, lib=lib, mode=mode)


@pytest.fixture(scope="module")
def frames(built):
    """per scene: the counters of the oracle's first pass, the first-hit instance of every pixel, and whether everything stays finite
    over 8 passes"""
    out = {}
    for name in T.NAMES:
        cam = T.flat_scene(name)[1]
        ref = _renderer(name)
        counters = ref.render(1, threads=THREADS, counted=True)
        instance = np.array([[ref.pick(x, y)[0] for x in range(cam.width)] for y in range(cam.height)])
        ref.render(T.PASSES - 1, threads=THREADS)
        finite = bool(np.isfinite(ref.accum).all() and all(np.isfinite(v).all() for v in ref.state.values()))
        out[name] = dict(counters=counters, instance=instance, finite=finite)
        ref.close()
    return out


def test_scene_list(built):
    """every base scene with lights and without, the two mask scenes with lights; frames at most 48x32, one partial tile, one 33x33"""
    assert len(set(T.NAMES)) == len(T.NAMES) == 2 * len(T.BASES) + len(T.MASKS)
    assert set(T.SHAPES) == set(T.BASES) | set(T.MASKS)
    sizes = {name: (T.flat_scene(name)[1].width, T.flat_scene(name)[1].height) for name in T.NAMES}
    assert set(sizes.values()) == {(48, 32), (33, 33), (5, 3)}
    for name in T.NAMES:
        flat, _, cfg, world, _ = T.flat_scene(name)
        lights = len(flat.spot_lights) + len(flat.direct_lights)
        assert lights == (0 if name.endswith("_sky") else 2), name
        assert (world.material.emission > 0) == name.endswith("_sky"), name
        assert (cfg.spot_samples, cfg.direct_samples) == (2, 1), name
        assert len(flat.tris) <= 1300, (name, len(flat.tris))


def test_every_scene_holds_its_shape_under_both_builders(built):
    backend = HostBackend(lib=oracle.load(), prefix="rzo_")
    print("\nscene                       Size nodes (depths)   non-root leaves > 8   root leaves > 8   deepest leaf   empty leaves")
    for name in T.NAMES:
        flat, world = T.flat_scene(name)[0], T.flat_scene(name)[3]
        stats = T.tree_stats(flat)
        assert T.SHAPES[_base(name)](stats), (name, stats)
        other = flatten(world, backend)
        assert T.tree_stats(other) == stats, f"{name}: the oracle's builder gives another tree"
        assert np.array_equal(other.nodes, flat.nodes) and np.array_equal(other.tris, flat.tris), name
        if not name.endswith("_sky"):
            print(f"{name:26s}  {stats['size_nodes']:2d} {sorted(stats['size_depths'])!s:14s}  {sorted(c for c in stats['leaves'].elements() if c > 8)!s:20s}  "
                  f"{sorted(c for c in stats['root_leaves'] if c > 8)!s:18s}  {stats['deepest_leaf']:4d}  {stats['empty_leaves']:4d}")


def test_world_trees(built):
    """root_leaf_N: a world of one leaf of at most 8 instances (what the one-leaf walk needs); root_leaves_world9: 9 or more"""
    for name in T.NAMES:
        flat = T.flat_scene(name)[0]
        root = int(flat.nodes[flat.tlas_root]["meta"])
        if _base(name) == "root_leaves_world9":
            assert len(flat.instances) >= 9 and not root & _abi.NODE_LEAF, name
        else:
            assert root & _abi.NODE_LEAF and (root & _abi.NODE_COUNT_MASK) == len(flat.instances) <= 8, name


def test_some_instances_are_mirrored_or_strongly_non_uniform(built):
    scales = [i.scale for name in T.NAMES if _base(name).startswith("big_leaf_") for i in T.flat_scene(name)[3].instances]
    assert sum(bool((s < 0).any()) for s in scales) >= 4 and sum(bool(np.abs(s).max() > 6 * np.abs(s).min()) for s in scales) >= 4


def test_coincident_triangles_sit_where_intended(built):
    """ties_across_chunks: the copies of one triangle are at positions 5, 13 and 69 of the 100-leaf (k, k + 8, k + 64), bit-equal in
    their vertices, and carry three different material slots"""
    for name in ("ties_across_chunks", "ties_across_chunks_sky"):
        flat = T.flat_scene(name)[0]
        copies = [40 + p for p in T.TIE_POSITIONS]               # the mesh lists its 40 grid triangles first
        where = T.leaf_positions(flat, set(copies))
        leaves = {where[c][0] for c in copies}
        assert len(leaves) == 1 and [where[c][1] for c in copies] == list(T.TIE_POSITIONS), where
        leaf = flat.nodes[leaves.pop()]
        assert int(leaf["meta"]) & _abi.NODE_COUNT_MASK == 100
        records = [flat.tris[int(leaf["begin"]) + p] for p in T.TIE_POSITIONS]
        for r in records[1:]:
            assert all(np.array_equal(r[v], records[0][v]) for v in ("v1", "v2", "v3"))
        slots = [int(r["material_flags"]) & _abi.TRI_MATERIAL_MASK for r in records]
        assert slots == [2, 1, 0], slots
        materials = [T.flat_scene(name)[3].instances[0].materials[s] for s in slots]
        assert materials[0].emission > 0 and materials[1].metalness > 0.5 and materials[2].emission == 0 and materials[2].metalness == 0


def test_mask_scenes_carry_a_partly_transparent_map(built):
    for name in T.MASKS:
        flat = T.flat_scene(name)[0]
        assert len(flat.textures) == 1
        alpha = flat.texels.reshape(-1, 4)[:, 3]
        assert (alpha == 0).any() and (alpha == 255).any() and ((alpha > 0) & (alpha < 255)).any()
        leaf = [n for n in flat.nodes if int(n["meta"]) & _abi.NODE_LEAF and (int(n["meta"]) & _abi.NODE_COUNT_MASK) > 64][0]
        records = flat.tris[int(leaf["begin"]):int(leaf["begin"]) + (int(leaf["meta"]) & _abi.NODE_COUNT_MASK)]
        assert ((records["material_flags"] & _abi.TRI_HAS_TEXCRDS) != 0).all() and ((records["material_flags"] & _abi.TRI_MATERIAL_MASK) == 3).all()


def test_the_validator_accepts_every_scene(built):
    from rayzath_amd import _lib
    lib = _lib.load()
    for name in T.NAMES:
        msg = C.create_string_buffer(256)
        assert lib.hiprz_validate_scene(C.byref(T.flat_scene(name)[0].struct), msg, 256) == 0, (name, msg.value.decode())


def test_oracle_frames_are_finite(frames):
    assert [name for name in T.NAMES if not frames[name]["finite"]] == []


def test_cameras_see_the_meshes(frames):
    """the first hit is an instance of the scene's mesh (any but the last instance, the receiver) on at least a quarter of the pixels"""
    for name in T.NAMES:
        receiver = len(T.flat_scene(name)[0].instances) - 1
        instance = frames[name]["instance"]
        share = float(((instance >= 0) & (instance < receiver)).mean())
        print(f"{name:26s} mesh {share:.2f}, receiver {float((instance == receiver).mean()):.2f}")
        assert share >= 0.25, (name, share)


def test_shadow_rays_test_triangles(frames):
    for name in T.NAMES:
        c = frames[name]["counters"]
        if name.endswith("_sky"):
            assert c["shadow_rays"] == 0 == c["shadow_tri_tests"], name
        else:
            assert c["shadow_rays"] > 0 and c["shadow_tri_tests"] > 0, (name, c)
        assert c["hits"] > 0 and c["tri_tests"] > c["shadow_tri_tests"], name


def test_same_name_gives_the_same_bytes(built):
    """world(name) is deterministic: built twice, the flattened arrays agree byte for byte"""
    for name in ("big_leaf_13", "size_chain_sky", "deep", "empty_leaf", "masks_65"):
        world, _ = T.world(name)
        again, flat = flatten(world), T.flat_scene(name)[0]
        for k in flat.FIELDS:
            assert getattr(again, k).tobytes() == getattr(flat, k).tobytes(), (name, k)


def test_a_box_may_refuse_a_triangle_that_is_nearer_by_a_rounding(built):
    """Why `deep` keeps its nearly coplanar triangles too small to be met (tree_shape_scenes.py): two triangles of its first version,
    across the x axis at x = 8^-9 and 8^-12, nearer to each other than an ulp of the hit distance.  With the reference's own arithmetic
    (rzo_triangle_test, rzo_box_test): where the first is hit at t and the second would be accepted below t, the second's OWN box is
    sometimes refused at far = t.  A tree that meets the second in a box of its own after the first reports the first; a tree that
    holds both in one leaf reports the second: the first-hit depth then depends on the tree's boxes, under any correct walk."""
    lib, f32 = oracle.load(), np.float32

    def blade(k, r, theta):
        x = f32(8.0) ** f32(-k)
        s, c, sn = x * f32(0.25), f32(r * np.cos(theta)), f32(r * np.sin(theta))
        return np.array([(x - s, -c, -sn), (x + s, c, sn), (x, c, -sn)], f32)

    def triangle(v, o, d, far):
        out = np.zeros(4, f32)
        hit = lib.rzo_triangle_test(v[0].ctypes.data, v[1].ctypes.data, v[2].ctypes.data, o.ctypes.data, d.ctypes.data, 1e-2, float(far), out.ctypes.data)
        return bool(hit), out[0]

    first, second = blade(9, 0.5, 0.7), blade(12, 0.45, 0.9)
    lo, hi = np.ascontiguousarray(second.min(0)), np.ascontiguousarray(second.max(0))
    rng = np.random.default_rng(7)
    both = refused = 0
    for _ in range(20000):
        o = np.array([3.0 + rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)], f32)
        d = np.array([0.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)], f32) - o
        d = (d / np.sqrt((d * d).sum(dtype=f32))).astype(f32)
        hit, t = triangle(first, o, d, 1e3)
        if not hit or not triangle(second, o, d, t)[0]:
            continue
        both += 1
        refused += not lib.rzo_box_test(lo.ctypes.data, hi.ctypes.data, o.ctypes.data, d.ctypes.data, 1e-2, float(t))
    print(f"the second triangle is nearer on {both} rays; its own box is refused at the first one's distance on {refused} of them")
    assert both > 1000 and refused > 10


def _flags(scene, lib, mode):
    dev, ref = _renderer(scene, lib=lib, mode=mode), _renderer(scene, mode=mode)
    r = lockstep.lockstep(OracleDevice(dev, threads=THREADS), ref, T.PASSES, records=0, threads=THREADS)
    dev.close(), ref.close()
    return bad(r), bool(bad(r) > lockstep.scene_cap(scene, mode, threads=THREADS) or r["depth_mismatch"])


@pytest.mark.parametrize("mutant,mode", [(m, 0) for m in MUTANTS] + [("shadow_sixtyfour", 31)])
def test_the_rule_flags_every_mutant_here_and_nowhere_in_the_old_sweep(built, mutant, mode):
    """A mutant oracle in the device's place breaks the rule the GPU is held to (discrete + far above the scene's cap, or a first-hit
    depth that differs) on the scenes built for its bug, and on no scene of generated_scenes.SEEDS: the older sweep could not have
    noticed a walk with this bug."""
    lib = oracle.variant("mut_" + mutant)
    here = {name: _flags(name, lib, mode) for name in T.NAMES}
    flagged = [name for name, (_, f) in here.items() if f]
    old = {seed: _flags(seed, lib, mode) for seed in G.SEEDS}
    print(f"mutant {mutant} mode {mode}: flagged on {len(flagged)} of {len(T.NAMES)} tree-shape scenes {flagged}, "
          f"{sum(n for n, _ in here.values())} discrete + far segments; on the generated scenes {[s for s, (_, f) in old.items() if f]}, "
          f"{sum(n for n, _ in old.values())} segments")
    for name in MUTANTS[mutant]:
        assert here[name][1], f"{mutant}: not flagged on {name}"
    assert [seed for seed, (_, f) in old.items() if f] == [], "the old sweep catches this mutant after all"
    assert sum(n for n, _ in old.values()) == 0
