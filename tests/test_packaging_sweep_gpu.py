"""Every launch packaging and every call pattern against the pass-by-pass render of the default packaging, bit for bit, over the generated
scenes of the lockstep sweep (tests/generated_scenes.py).

tests/test_lockstep_gpu.py ties the default packaging rendered one pass per call ("default", and "compat31-split" for the CUDA-compat
integrator) to the CPU oracle, segment by segment.  Every packaging of the library is specified to give the same frame bit for bit, so
this file asserts exactly that and nothing weaker: per scene the BASELINE is render(1) eight times under default settings (mode 31 for
the compat variants); every VARIANT renders the scene with the call patterns (8,), (1, 2, 5) and (3, 5), and after every call that ends
on 1, 3 or 8 passes the accumulator, the first-hit depth, every read_state() field, ray_count() and pass_count() equal the baseline's
(tests/packaging_sweep.py).  That carries the oracle comparison to chains of passes inside one launch — rz_batch_kernel with the path
state parked in LDS, rz_batch_seg_kernel handing it through memory, rz_wave_batch_kernel's per-wave chains, launches in the cost order
of the launch before — and to every kernel instantiation a plan can name, at zero tolerance and without running the oracle again.

Which instantiation a variant really launched is read back (Context.launch_plan -> test_launch_plan.kernel_identities) and the last test
holds the union against tests/golden/launch_plan/identities.txt, the identities of the 2.4 M plans tests/test_launch_plan.py walks.

Where a knob of the issue's list is inert without a second one, the variant sets both: HIPRZ_TRACE_WAVES, the walk order, the ray sort and
the shadow walks only act on the skip-link walks (mode 3), which a scene small enough to be staged selects only when asked
(set_traversal_mode(3), the "split-global" packaging of test_shading_inputs_gpu.PACKAGINGS); "split-global-plain" is the combination
without it, the workgroup trace kernel on the global scene.

Run with -s for the identities per variant and the counts of the closing test; the measured figures are in DESIGN.md (Oracle, "Lockstep").
"""
import time

import numpy as np
import pytest

import generated_scenes as G
import lockstep
import packaging_sweep as S
from rayzath_amd.engine import Context
from test_launch_plan import identity_line, kernel_identities, read_identities

pytestmark = pytest.mark.gpu

CHUNK = 10
SCENES = G.SEEDS + G.DERIVED                  # the sweep's 60 scenes, and the scenes without lights / without maps derived from them
CHUNKS = [G.SEEDS[i:i + CHUNK] for i in range(0, len(G.SEEDS), CHUNK)] + [G.DERIVED]
ENV = ("HIPRZ_BATCH_SEGMENTS", "HIPRZ_BATCH_WAVES", "HIPRZ_HEAVY_FIRST", "HIPRZ_TRACE_WAVES", "HIPRZ_SHADOW_PACKET", "HIPRZ_SHADOW_TREE",
       "HIPRZ_SHADOW_SORT", "HIPRZ_DEFER_SHADOWS", "HIPRZ_SORT_BITS", "HIPRZ_NOLIGHT_KERNELS", "HIPRZ_WAVE_RESIDENT_MAX", "HIPRZ_SORT_KEY",
       "HIPRZ_WORLD_ADVANCE", "HIPRZ_WALK_ADVANCE")
BASELINES = {"default": {}, "compat31": dict(mode=31)}   # lockstep's "default" and "compat31-split", rendered pass by pass
OWN = "own"   # baseline of a variant that legitimately renders another frame: its own settings, rendered pass by pass (and in lockstep's CONFIGS)


def _variant(baseline="default", devices=0, env=None, config_seed=0, **settings):
    return dict(baseline=baseline, devices=devices, env=env or {}, config_seed=config_seed, settings=settings)


GLOBAL = dict(pipeline=1, lds_scene=0)        # split pipeline, scene not staged in LDS
SKIP = dict(GLOBAL, traversal_mode=3)         # ... walked on skip links by single-wave workgroups
VARIANTS = {
    # resident: the first-pass kernel, then chains of passes in one launch
    "default": _variant(),
    **{f"segments-{s}": _variant(env={"HIPRZ_BATCH_SEGMENTS": str(s)}) for s in (1, 2, 3, 8)},
    "batch-waves-4": _variant(env={"HIPRZ_BATCH_WAVES": "4"}),
    "heavy-first-0": _variant(env={"HIPRZ_HEAVY_FIRST": "0"}),
    "xcd-swizzle": _variant(xcd_swizzle=True),
    "xcd-swizzle-segments-3": _variant(env={"HIPRZ_BATCH_SEGMENTS": "3"}, xcd_swizzle=True),
    "mode-1": _variant(traversal_mode=1),
    "mode-2": _variant(traversal_mode=2),
    "mode-1-segments-2": _variant(env={"HIPRZ_BATCH_SEGMENTS": "2"}, traversal_mode=1),
    "mode-2-segments-2": _variant(env={"HIPRZ_BATCH_SEGMENTS": "2"}, traversal_mode=2),
    "resident-global": _variant(pipeline=2, lds_scene=0),   # no lights: the per-wave resident kernel; lights: the unstaged workgroup kernel
    "resident-global-tree-3": _variant(pipeline=2, lds_scene=0, tree=3),
    "resident-global-mode-1": _variant(pipeline=2, lds_scene=0, traversal_mode=1),
    "resident-global-mode-2": _variant(pipeline=2, lds_scene=0, traversal_mode=2),
    "resident-global-mode-1-segments-2": _variant(env={"HIPRZ_BATCH_SEGMENTS": "2"}, pipeline=2, lds_scene=0, traversal_mode=1),
    "resident-global-mode-2-segments-3": _variant(env={"HIPRZ_BATCH_SEGMENTS": "3"}, pipeline=2, lds_scene=0, traversal_mode=2),
    # the resident kernels on a staged scene wherever the blob fits LDS at all (set_lds_scene(1)): by itself a scene without lights is
    # staged AND resident only below 11 KiB of records, and no scene without lights that carries a map is that small
    "resident-lds-mode-1": _variant(pipeline=2, lds_scene=1, traversal_mode=1),
    "resident-lds-mode-2": _variant(pipeline=2, lds_scene=1, traversal_mode=2),
    "resident-lds-mode-1-segments-3": _variant(env={"HIPRZ_BATCH_SEGMENTS": "3"}, pipeline=2, lds_scene=1, traversal_mode=1),
    "resident-lds-mode-2-segments-2": _variant(env={"HIPRZ_BATCH_SEGMENTS": "2"}, pipeline=2, lds_scene=1, traversal_mode=2),
    "two-streams": _variant(devices=[0, 0]),
    # fused: one kernel per pass
    "fused": _variant(pipeline=0),
    "fused-global": _variant(pipeline=0, lds_scene=0),
    "fused-mode-1": _variant(pipeline=0, traversal_mode=1),
    "fused-mode-2": _variant(pipeline=0, traversal_mode=2),
    "fused-global-mode-1": _variant(pipeline=0, lds_scene=0, traversal_mode=1),
    "fused-global-mode-2": _variant(pipeline=0, lds_scene=0, traversal_mode=2),
    # split, staged
    "split-lds": _variant(pipeline=1),
    "split-lds-mode-1": _variant(pipeline=1, traversal_mode=1),
    "split-lds-mode-2": _variant(pipeline=1, traversal_mode=2),
    "split-lds-forced": _variant(pipeline=1, lds_scene=1),   # the larger scenes without lights staged too (shade kernel without next-event estimation on a staged scene)
    # split, not staged
    "split-global-plain": _variant(**GLOBAL),
    "split-global-mode-1": _variant(**GLOBAL, traversal_mode=1),
    "split-global-mode-2": _variant(**GLOBAL, traversal_mode=2),
    "split-global": _variant(**SKIP),
    "walk-order-0": _variant(**SKIP, walk_order=0),
    **{f"trace-waves-{w}-walk-order-{o}": _variant(env={"HIPRZ_TRACE_WAVES": str(w)}, **SKIP, walk_order=o) for w in (5, 6) for o in (1, 0)},
    "shadow-packet-1": _variant(env={"HIPRZ_SHADOW_PACKET": "1"}, **SKIP),
    "shadow-packet-0": _variant(env={"HIPRZ_SHADOW_PACKET": "0"}, **SKIP),
    "shadow-packet-1-shadow-tree-0": _variant(env={"HIPRZ_SHADOW_PACKET": "1", "HIPRZ_SHADOW_TREE": "0"}, **SKIP),
    "shadow-sort-0": _variant(env={"HIPRZ_SHADOW_SORT": "0"}, **SKIP),
    "defer-shadows-0": _variant(env={"HIPRZ_DEFER_SHADOWS": "0"}, **SKIP),
    "ray-sort-0": _variant(**SKIP, ray_sort=0),
    "ray-sort-1": _variant(**SKIP, ray_sort=1),
    **{f"sort-bits-{b}": _variant(env={"HIPRZ_SORT_BITS": str(b)}, **SKIP, ray_sort=1) for b in (8, 16, 24)},
    "graph-on": _variant(**SKIP, graph=True),
    "graph-off": _variant(**SKIP, graph=False),
    **{f"tree-{t}": _variant(**GLOBAL, tree=t) for t in (1, 2, 3, 4)},
    # the CUDA-compat integrator, flags 31
    "compat31": _variant("compat31", mode=31),
    "compat31-shadow-packet-0": _variant("compat31", env={"HIPRZ_SHADOW_PACKET": "0"}, mode=31),
    # Four variants that differ from "compat31" in the accumulator's last bits on scenes where a shadow ray crosses several transparent
    # triangles (seeds 12 and 20), and legitimately: under HIPRZ_COMPAT_SHADOW_COLOR (flag 4 of 31) a shadow ray's mask is the PRODUCT of
    # the opacity colours of the triangles it crosses, multiplied in the order the walk meets them, and the walk stops once the mask's
    # alpha is below 1e-4 (hiprz_compat.hpp: compat_shadow_mask, `own = own * compat_crossing_color(...)`, `mask = mask * own`;
    # hiprz_device.hpp: any_hit_coop_mask does the same per wave).  Float products round per step, so another order gives other last
    # bits, and another set of factors before the stop.  The baseline's deferred rays walk front to back on skip links (SHADOWS_COOP3_COLOUR);
    # the fused kernel and HIPRZ_DEFER_SHADOWS=0 walk inline in the reference's child order, the beams (SHADOWS_PACKET_COLOUR) in the
    # wave's order over the shadow rays' own world tree, and device-built trees hold the triangles in another order altogether.  Path
    # state, depth and counters are equal everywhere; only `accum` differs.  Each is in test_lockstep_gpu.CONFIGS, held to the oracle
    # directly, and here to its own pass-by-pass render.
    "compat31-fused": _variant(OWN, mode=31, pipeline=0),
    "compat31-shadow-packet-1": _variant(OWN, env={"HIPRZ_SHADOW_PACKET": "1"}, mode=31),
    "compat31-defer-shadows-0": _variant(OWN, env={"HIPRZ_DEFER_SHADOWS": "0"}, mode=31),
    "compat31-tree-3": _variant(OWN, mode=31, tree=3),
}
# the harness must be able to fail: the same packaging as "default" on another random stream
ANOTHER_FRAME = _variant(config_seed=1)

# identity -> why the sweep does not have to reach it.  Only: the 5-wave batch kernel (batch.five == 1: plan_batch wants a grid of more
# than 2 560 tiles, the sweep's largest frame has 10; tests/test_batch_segments_gpu.py runs it on config B at full size), and identities
# that no context can produce, each with the rule that rules it out.
EXEMPT = {i: "batch.five: plan_batch needs more than 2 560 tiles; test_batch_segments_gpu.py covers it on B at full size"
          for i in read_identities() if i[0] == "batch" and i[5] == 1}

_BASELINE, _RESULTS, _SECONDS = {}, {}, {}


def _context(spec, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in spec["env"].items():
        monkeypatch.setenv(k, v)
    ctx = Context(spec["devices"])
    for k, v in spec["settings"].items():
        getattr(ctx, "set_" + k)(v)
    return ctx


def _scenes(chunk):
    """a chunk of this file's sweep by its index, or a tuple of scenes as it stands (tests/test_tree_shapes_gpu.py)"""
    return CHUNKS[chunk] if isinstance(chunk, int) else chunk


def _upload(ctx, seed, config_seed=0):
    flat, cam, cfg = lockstep.flat_scene(seed)[:3]
    if config_seed:
        cfg = type(cfg).from_buffer_copy(cfg)
        cfg.seed += config_seed
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)


def baseline(name, chunk, monkeypatch):
    """{seed: pass-by-pass frames} of one baseline over one chunk, rendered once and never written to again"""
    key = (name, chunk)
    if key not in _BASELINE:
        ctx, out = _context(_variant(**BASELINES[name]) if name in BASELINES else VARIANTS[name], monkeypatch), {}
        for seed in _scenes(chunk):
            _upload(ctx, seed)
            out[seed] = S.pass_by_pass(ctx)
            for snap in out[seed].values():
                for v in snap.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
        ctx.close()
        _BASELINE[key] = out
    return _BASELINE[key]


def run_chunk(name, chunk, monkeypatch, spec=None):
    """one context, the chunk's scenes one after the other, every call pattern on each:
    {seed: dict(differences=[...], identities={...})}; rendered once per (variant, chunk)"""
    key = (name, chunk)
    if key in _RESULTS:
        return _RESULTS[key]
    spec = spec or VARIANTS[name]
    want = baseline(name if spec["baseline"] == OWN else spec["baseline"], chunk, monkeypatch)
    start = time.perf_counter()
    ctx, out = _context(spec, monkeypatch), {}
    for seed in _scenes(chunk):
        _upload(ctx, seed, spec["config_seed"])
        diff = S.compare_patterns(ctx, want[seed])
        out[seed] = dict(differences=diff, identities=kernel_identities(ctx.launch_plan()))
    ctx.close()
    _SECONDS[key] = time.perf_counter() - start
    _RESULTS[key] = out
    return out


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_packaging_sweep(built, monkeypatch, name, chunk):
    results = run_chunk(name, chunk, monkeypatch)
    reached = sorted(set().union(*[r["identities"] for r in results.values()]))
    print(f"packaging sweep {name} chunk {chunk}: {_SECONDS[(name, chunk)]:.2f} s, identities: " + "; ".join(identity_line(i) for i in reached))
    failures = [f"seed {seed} calls {calls} after {passes} passes: {field} differs ({what})"
                for seed, r in results.items() for calls, passes, field, what in r["differences"]]
    assert not failures, f"{name}: {len(failures)} differences from the pass-by-pass render\n" + "\n".join(failures[:40])


def test_launch_plan_accessor(built):
    """hiprz_launch_plan: refused before the first render call and with a short or missing buffer; afterwards the words of the plan of the
    last call, on a context over two streams the head part's; reading it changes nothing."""
    import ctypes as C
    from rayzath_amd import _abi
    from rayzath_amd.engine import HiprzError
    from test_launch_plan import plan_dtype
    for devices in (0, [0, 0]):
        ctx = Context(devices)
        _upload(ctx, 0)
        with pytest.raises(HiprzError) as e:
            ctx.launch_plan()
        assert e.value.code == _abi.ERR_STATE
        ctx.render(1)
        words, n = (C.c_uint32 * 64)(), C.c_uint32(0)
        assert ctx.lib.hiprz_launch_plan(ctx._ctx, None, 64, C.byref(n)) == _abi.ERR_INVALID
        assert ctx.lib.hiprz_launch_plan(ctx._ctx, words, 64, None) == _abi.ERR_INVALID
        assert ctx.lib.hiprz_launch_plan(ctx._ctx, words, plan_dtype.itemsize // 4 - 1, C.byref(n)) == _abi.ERR_INVALID
        assert n.value == 0 and not any(words)
        before = S.snapshot(ctx)
        plan = ctx.launch_plan()
        assert plan.dtype == np.uint32 and plan.nbytes == plan_dtype.itemsize
        record = plan.view(plan_dtype)[0]
        cam = G.flat_scene(0)[1]
        tiles = ((cam.width + 31) // 32) * ((cam.height + 7) // 8)
        pipeline = ctx.pipeline()   # whatever this scene resolves to by itself
        assert record["pipeline"] == pipeline and record["reported_mode"] == ctx.traversal_mode()
        assert record["tile_grid"] == (tiles if devices == 0 else (tiles + 1) // 2), "the head part owns every second tile"
        assert bool(record["batch.family"]) == (pipeline == 2) and bool(record["fused.family"]) != bool(record["trace.family"])
        assert record["shade.active"] == bool(record["trace.family"])
        assert np.array_equal(ctx.launch_plan(), plan) and S.differences({1: S.snapshot(ctx)}, {1: before}) == []
        other = 0 if pipeline else 1
        ctx.set_pipeline(other)
        assert np.array_equal(ctx.launch_plan(), plan), "a setter alone computes no plan"
        ctx.render(2)
        after = ctx.launch_plan().view(plan_dtype)[0]
        assert after["pipeline"] == other == ctx.pipeline() and bool(after["fused.family"]) == (other == 0) and not after["batch.family"]
        ctx.close()


def test_sweep_notices_another_frame(built, monkeypatch):
    """The default packaging on the random stream of config seed + 1 in the variant's place: the comparison reports it on every scene
    whose world is not empty (an empty world's frame is the sky's, which may be constant)."""
    for chunk in range(len(CHUNKS)):
        results = run_chunk("another-frame", chunk, monkeypatch, spec=ANOTHER_FRAME)
        for seed, r in results.items():
            if G.flat_scene(seed)[3].instances:
                assert r["differences"], f"seed {seed}: another random stream, and nothing differs"


def test_sweep_reaches_every_kernel_identity(built, monkeypatch):
    """reached + EXEMPT is the whole list of tests/golden/launch_plan/identities.txt, nothing exempt is reached, and every identity
    that is not exempt is reached on at least 3 scenes (the floor generated_scenes.FEATURES uses)."""
    universe = read_identities()
    reached = {}                                   # identity -> {(variant, seed)}
    for name in VARIANTS:
        for chunk in range(len(CHUNKS)):
            for seed, r in run_chunk(name, chunk, monkeypatch).items():
                for identity in r["identities"]:
                    reached.setdefault(identity, set()).add((name, seed))
    slowest = max(_SECONDS, key=_SECONDS.get)
    print(f"packaging sweep: {len(reached)} identities reached, {len(EXEMPT)} exempt, {len(universe)} in identities.txt; "
          f"{len(VARIANTS)} variants x {len(CHUNKS)} chunks in {sum(_SECONDS.values()):.1f} s, slowest case {slowest} {_SECONDS[slowest]:.2f} s")
    for identity in sorted(universe):
        pairs = reached.get(identity, set())
        print(f"  {identity_line(identity):28s} {len(pairs):5d} (variant, seed) pairs, {len({s for _, s in pairs}):2d} seeds, {len({v for v, _ in pairs}):2d} variants"
              + (f"   exempt: {EXEMPT[identity]}" if identity in EXEMPT else ""))
    assert set(EXEMPT) <= universe, sorted(set(EXEMPT) - universe)
    assert not set(reached) & set(EXEMPT), f"exempt, yet reached: {sorted(set(reached) & set(EXEMPT))}"
    assert set(reached) | set(EXEMPT) == universe, (f"never reached: {sorted(universe - set(reached) - set(EXEMPT))}, "
                                                    f"not in identities.txt: {sorted(set(reached) - universe)}")
    thin = {identity_line(i): sorted({s for _, s in pairs}, key=str) for i, pairs in reached.items() if len({s for _, s in pairs}) < 3}
    assert not thin, f"reached on fewer than 3 scenes: {thin}"
