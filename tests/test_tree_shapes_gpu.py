"""Every walk of the library over the tree shapes of tests/tree_shape_scenes.py — Size nodes, leaves of 9 to 300 triangles below a mesh's
root, root leaves above 32, coincident triangles 8 and 64 positions apart, a tree 21 deep, empty leaves and the depth-limit leaf — held to
the CPU oracle exactly, with the harnesses of the two older sweeps and nothing new:

  lockstep        tests/lockstep.py, one path segment per pixel from the device's own state, 8 passes, under every packaging of
                  test_shading_inputs_gpu.PACKAGINGS x modes 0, 31, 63 x the uploaded reference trees and set_tree(1), (2), (3).  The bar
                  is test_lockstep_gpu's: discrete + far <= lockstep.scene_cap (from the libm stand-ins on that scene), first-hit depth
                  bit-equal, ray and pass counts equal.
                  A 48x32 frame takes the cooperative shadow walk by itself, so the scenes with lights run again with the wave-level walk
                  (HIPRZ_SHADOW_PACKET=1; modes 0, 31, 63) and with inline shadow rays (HIPRZ_DEFER_SHADOWS=0; modes 0, 31), on trees 0
                  and 3, and the launch plan is read back to see that the walk asked for ran.
  counters        one counted first pass: on the reference-order walk (pipeline 1, walk order 0, scene not staged) EVERY counter equals
                  the oracle's — each triangle of a 257-leaf is tested once per ray that enters it —; on the packagings above segments,
                  hits, finished paths, light samples and shadow rays do, and the box and triangle tests net of the shadow rays'.
  packaging sweep tests/packaging_sweep.py under every entry of test_packaging_sweep_gpu.VARIANTS (the shadow walks forced both ways and
                  onto the reference's world tree among them) and under the three HIPRZ_WORLD_ADVANCE / HIPRZ_WALK_ADVANCE settings of
                  test_world_levels_gpu, bit for bit against the pass-by-pass render.
  one-leaf walk   root_leaf_N in a world of three instances: the default traversal on pipelines 2, 0 and 1 against the
                  set_traversal_mode(1) twin, by test_packed_pairs_gpu.compare_with_the_stack_walk.
  other users     hiprz_read_guides (depth, instance) and hiprz_pick on a lattice of pixels against the first pass's depth and the
                  oracle's first-hit instance.

Run with -s: the closing test prints, per scene, how many lockstep configurations and sweep variants ran on it and its slowest case.

Measured on MI355X: 749 cases in 203 s (288 + 30 lockstep, 408 sweep, 6 counters, 8 one-leaf, 6 guides, 2 builds), beside 68 s for
test_packaging_sweep_gpu.py and 15 s for test_lockstep_gpu.py; the slowest case takes 3.6 s (the first of a chunk, which also computes
the stand-ins' caps of its scenes on the CPU).  On the uploaded reference trees, on host SAH trees and on the device's
Morton trees every case passes: every walk meets every triangle of every leaf, the reference's first of coincident triangles wins, and
the reference-order walk's counters equal the oracle's to the last shadow triangle test.

TWO FINDINGS, both on set_tree(3), the device's binned surface-area builder, both fixed with this file:
  * The build was not reproducible.  The same mesh uploaded into fresh contexts gave the same nodes and ANOTHER order of the triangles
    inside the leaves when many triangles share one centre: 128 to 192 of masks_257's positions, 128 of big_leaf_257's, 124 to 244 of
    root_leaf_300's differed between two uploads.  A node that no plane separates was cut in half "as its run stands", and the run
    stood as the atomic cursors of the levels above had left it.  Minimum and any-hit do not care; the coloured shadow masks of mode 31
    are products in the order a walk meets the triangles, so test_packaging_sweep[compat31-tree-3-5] found 4 (after 3 passes) and 23 or
    24 (after 8) of masks_257's 6 144 accumulator values in other last bits than the same settings rendered pass by pass in another
    context.  rz_sah_partition_kernel now takes the lower half by triangle index (test_device_trees_are_the_same_at_every_upload;
    test_device_tree_audit_gpu.py holds such meshes to the numpy reference); above 8 192 triangles in one halved node the run's order still decides.
  * rz_compat_pass_kernel walked without the tie rule (closest_hit_skip's TIES), so on a rebuilt tree the fused compat kernel picked the
    coincident triangle its tree's order met first, not the reference's: test_lockstep[fused-31-3-*] and [fused-63-3-*] showed
    0 discrete + 1 044 far segments of 12 288 on ties_across_chunks and ties_across_chunks_sky (cap 2) in one run and none in the run
    before it, with the order the build happened to give.  It now ranks equal distances by reference position like every other walk.
"""
import time

import numpy as np
import pytest

import lockstep
import oracle
import test_lockstep_gpu as L
import test_packaging_sweep_gpu as P
import tree_shape_scenes as T
from lockstep import bad
from rayzath_amd import _abi
from rayzath_amd.engine import COMPAT_REPROJECTION, Context
from test_launch_plan import identity_line, kernel_identities
from test_packed_pairs_gpu import compare_with_the_stack_walk
from test_shading_inputs_gpu import PACKAGINGS

pytestmark = pytest.mark.gpu

THREADS = 8                    # of the oracle's; its frames do not depend on the count
CHUNK = 8
CHUNKS = [T.NAMES[i:i + CHUNK] for i in range(0, len(T.NAMES), CHUNK)]
MODES = (0, 31, 63)
TREES = (0, 1, 2, 3)
REFERENCE_ORDER = dict(pipeline=1, walk_order=0, lds_scene=0)
ADVANCES = {f"advance-{w}-{i}": P._variant(env={"HIPRZ_WORLD_ADVANCE": w, "HIPRZ_WALK_ADVANCE": i}, tree=3) for w, i in (("0", "0"), ("1", "3"), ("64", "64"))}
SWEEP = {**P.VARIANTS, **ADVANCES}
_LOCKSTEP, _SECONDS, _RAN = {}, {}, {}


def _note(scene, kind, label, seconds):
    _RAN.setdefault(scene, {}).setdefault(kind, set()).add(label)
    _SECONDS[(scene, kind, label)] = seconds


def _settings(packaging, mode, tree):
    out = dict(PACKAGINGS[packaging])
    if mode:
        out["mode"] = mode
    if tree:
        out["tree"] = tree
    return out


def run_lockstep(label, settings, mode, scenes, env=None):
    """one context (created under `env`), the scenes uploaded one after the other (mode 63: a context per scene, as in test_lockstep_gpu):
    {scene: result}"""
    key = (label, scenes)
    if key in _LOCKSTEP:
        return _LOCKSTEP[key]
    config, out = dict(settings=settings, env=env or {}), {}
    ctx = L._context(config)
    for name in scenes:
        start = time.perf_counter()
        flat, cam, cfg = T.flat_scene(name)[:3]
        if mode & COMPAT_REPROJECTION:
            ctx.close()
            ctx = L._context(config)
        ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
        ref = oracle.OracleRenderer(flat, cam, cfg, mode=mode)
        result = lockstep.lockstep(ctx, ref, T.PASSES, threads=THREADS)
        result["rays"] = (ctx.ray_count(), ref.traced_rays)
        result["passes"] = (ctx.pass_count(), ref.passes)
        result["tree"] = ctx.tree()
        result["identities"] = kernel_identities(ctx.launch_plan())
        ref.close()
        out[name] = result
        _note(name, "lockstep", label, time.perf_counter() - start)
    ctx.close()
    _LOCKSTEP[key] = out
    return out


def _hold_to_the_rule(results, label, mode, tree):
    failures = []
    for name, r in results.items():
        cap = lockstep.scene_cap(name, mode, threads=THREADS)
        print(f"lockstep {label} {name}: {r['segments']} segments, exact {r['exact']}, far {r['far']}, discrete {r['discrete']}, cap {cap}")
        assert r["tree"] == tree, (name, r["tree"])
        L._check_depth(r, name, mode)
        cam = T.flat_scene(name)[1]
        assert r["rays"][0] == r["rays"][1] == T.PASSES * cam.width * cam.height, (name, r["rays"])
        assert r["passes"][0] == r["passes"][1] == T.PASSES, (name, r["passes"])
        if bad(r) > cap:
            failures.append(f"{name}: {r['discrete']} discrete + {r['far']} far segments, cap {cap}\n{lockstep.describe(r)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("packaging", list(PACKAGINGS))
def test_lockstep(built, packaging, mode, tree, chunk):
    label = f"{packaging} mode {mode} tree {tree}"
    _hold_to_the_rule(run_lockstep(label, _settings(packaging, mode, tree), mode, CHUNKS[chunk]), label, mode, tree)


# The shadow walks a 48x32 frame does not choose by itself, each held to the oracle directly (the packaging sweep compares the compat
# modes' coloured masks only with the same walk rendered pass by pass: products in another order agree to rounding, not to the bit).
# "beams": the wave-level walk any_hit_packet (mode 0: SHADOWS_PACKET on the skip-link packaging; compat: SHADOWS_PACKET_COLOUR, the
# colour hand-over across 64-pair steps and both divisions); "inline": HIPRZ_DEFER_SHADOWS=0, the shadow rays walked inside the shade
# kernel (compat_shadow_mask).  Scenes with lights only.
LIT = tuple(n for n in T.NAMES if not n.endswith("_sky"))
LIT_CHUNKS = [LIT[i:i + 9] for i in range(0, len(LIT), 9)]
SHADOW_WALKS = {"beams": ({"HIPRZ_SHADOW_PACKET": "1"}, (0, 31, 63)), "inline": ({"HIPRZ_DEFER_SHADOWS": "0"}, (0, 31))}
FOLLOW_PACKET, FOLLOW_PACKET_COLOUR = 1, 2   # SHADOWS_PACKET, SHADOWS_PACKET_COLOUR of hiprz_plan.hpp


@pytest.mark.parametrize("chunk", range(len(LIT_CHUNKS)))
@pytest.mark.parametrize("tree", (0, 3))
@pytest.mark.parametrize("walk,mode", [(w, m) for w, (_, modes) in SHADOW_WALKS.items() for m in modes])
def test_lockstep_forced_shadow_walks(built, walk, mode, tree, chunk):
    label = f"shadow {walk} mode {mode} tree {tree}"
    settings = dict(mode=mode) if mode else dict(PACKAGINGS["split-global"])   # mode 0: the shadow walks act on the skip-link walks only
    if tree:
        settings["tree"] = tree
    results = run_lockstep(label, settings, mode, LIT_CHUNKS[chunk], env=SHADOW_WALKS[walk][0])
    for name, r in results.items():   # the walk that was asked for is the one that ran
        follow = {i[1] for i in r["identities"] if i[0] == "follow"}
        assert follow == ({FOLLOW_PACKET_COLOUR if mode else FOLLOW_PACKET} if walk == "beams" else set()), (name, r["identities"])
    _hold_to_the_rule(results, label, mode, tree)


def _first_pass(settings, name):
    flat, cam, cfg = T.flat_scene(name)[:3]
    ctx = Context(0)
    for k, v in settings.items():
        getattr(ctx, "set_" + k)(v)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    counters, depth = ctx.render_counted(1), ctx.read_depth()
    ctx.close()
    return counters, depth


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_counters_of_the_first_pass(built, chunk):
    """the reference-order walk tests what the oracle tests, box for box and triangle for triangle, shadow rays included; the other
    packagings walk in another order (their shadow rays stop at another triangle) and agree in everything else"""
    for name in CHUNKS[chunk]:
        flat, cam, cfg = T.flat_scene(name)[:3]
        ref = oracle.OracleRenderer(flat, cam, cfg)
        want = ref.render(1, threads=THREADS, counted=True)
        want_depth = ref.depth
        ref.close()
        got, depth = _first_pass(REFERENCE_ORDER, name)
        print(f"counters {name}: reference-order walk {got}\n{' ' * (10 + len(name))}oracle               {want}")
        assert np.array_equal(depth, want_depth), name
        assert got == want, (name, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        for packaging, settings in PACKAGINGS.items():
            got, depth = _first_pass(settings, name)
            print(f"counters {name}: {packaging} {got}")
            assert np.array_equal(depth, want_depth), (name, packaging)
            for k in ("segments", "hits", "finished", "light_samples", "shadow_rays", "texel_fetches"):
                assert got[k] == want[k], (name, packaging, k, got[k], want[k])
            for total, shadow in (("box_tests", "shadow_box_tests"), ("tri_tests", "shadow_tri_tests")):
                assert got[total] - got[shadow] == want[total] - want[shadow], (name, packaging, total)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("variant", list(SWEEP))
def test_packaging_sweep(built, monkeypatch, variant, chunk):
    scenes = CHUNKS[chunk]
    start = time.perf_counter()
    results = P.run_chunk(variant, scenes, monkeypatch, spec=SWEEP[variant])
    seconds = time.perf_counter() - start
    for name in scenes:
        _note(name, "sweep", variant, seconds / len(scenes))
    reached = sorted(set().union(*[r["identities"] for r in results.values()]))
    print(f"packaging sweep {variant} scenes {scenes[0]} .. {scenes[-1]}: {seconds:.2f} s (with the baseline where it was not rendered yet), "
          f"identities: " + "; ".join(identity_line(i) for i in reached))
    failures = [f"{name} calls {calls} after {passes} passes: {field} differs ({what})"
                for name, r in results.items() for calls, passes, field, what in r["differences"]]
    assert not failures, f"{variant}: {len(failures)} differences from the pass-by-pass render\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("name", [n for n in T.NAMES if n.startswith("root_leaf_")])
def test_one_leaf_walk_beyond_32_triangles(built, name):
    flat, cam, cfg = T.flat_scene(name)[:3]
    root = int(flat.nodes[flat.tlas_root]["meta"])
    assert root & _abi.NODE_LEAF and (root & _abi.NODE_COUNT_MASK) == len(flat.instances) <= 8
    assert max(T.tree_stats(flat)["root_leaves"]) == int(name.split("_")[2]) > 32
    compare_with_the_stack_walk(name, flat, cam, cfg)


@pytest.mark.parametrize("tree", (2, 3))
def test_device_trees_are_the_same_at_every_upload(built, tree):
    """meshes of 257 and 300 triangles that share one centre, uploaded into three fresh contexts (once behind other scenes): the same
    nodes and the same triangle order in the leaves each time"""
    def trees(names):
        ctx, out = Context(0), {}
        ctx.set_tree(tree)
        for name in names:
            flat, cam, cfg = T.flat_scene(name)[:3]
            ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
            nodes, _, _, roots, refpos = ctx.download_trees(len(flat.instances), len(flat.tris), len(flat.tlas_order))
            out[name] = (nodes.tobytes(), roots.tobytes(), refpos.tobytes())
        ctx.close()
        return out
    names = ("masks_257", "big_leaf_257", "root_leaf_300", "ties_across_chunks")
    first = trees(names)
    assert trees(names) == first
    behind = trees(("big_leaf_300", "masks_65") + names[::-1])
    assert all(behind[name] == first[name] for name in names)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_guides_and_pick(built, chunk):
    ctx = Context(0)
    for name in CHUNKS[chunk]:
        flat, cam, cfg = T.flat_scene(name)[:3]
        ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
        ref = oracle.OracleRenderer(flat, cam, cfg)
        ctx.render(1), ref.render(1, threads=THREADS)
        depth, guides = ctx.read_depth(), ctx.read_guides()
        assert np.array_equal(depth.view(np.uint32), ref.depth.view(np.uint32)), name
        assert np.array_equal(guides["depth"].view(np.uint32), depth.view(np.uint32)), name
        xs = sorted(set(np.linspace(0, cam.width - 1, 12).astype(int).tolist()))
        ys = sorted(set(np.linspace(0, cam.height - 1, 8).astype(int).tolist()))
        hits = 0
        for y in ys:
            for x in xs:
                want = ref.pick(x, y)
                assert ctx.pick(x, y) == want, (name, x, y)
                instance = int(guides[y, x]["instance"])
                assert (instance == want[0]) if want[0] >= 0 else (instance == _abi.GUIDE_MISS), (name, x, y, instance, want)
                hits += want[0] >= 0
        assert hits >= len(xs) * len(ys) // 2, name
        ref.close()
    ctx.close()


def test_what_ran(built):
    """per scene: the lockstep configurations and sweep variants that ran on it in this process, and its slowest case (a sweep variant's
    time is its chunk's, divided by the chunk's scenes)"""
    for name in T.NAMES:
        ran = _RAN.get(name, {})
        mine = {k: v for k, v in _SECONDS.items() if k[0] == name}
        slowest = max(mine, key=mine.get) if mine else None
        print(f"{name:26s} lockstep configurations {len(ran.get('lockstep', ())):3d}, sweep variants {len(ran.get('sweep', ())):3d}" +
              (f", slowest {slowest[1]} {slowest[2]}: {mine[slowest]:.2f} s" if slowest else ""))
    print(f"lockstep {sum(v for k, v in _SECONDS.items() if k[1] == 'lockstep'):.1f} s, sweep {sum(v for k, v in _SECONDS.items() if k[1] == 'sweep'):.1f} s")
