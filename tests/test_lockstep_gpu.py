"""The HIP kernels against the CPU oracle in lockstep (tests/lockstep.py) over the generated scenes (tests/generated_scenes.py): every pass
the oracle continues from the device's own accumulator and path state, so each pass compares one path segment per pixel from bit-identical
inputs.  Configurations: every packaging of test_shading_inputs_gpu.PACKAGINGS, a two-stream context, the device-built trees, and the
CUDA-compat integrator (modes 31 and 63, fused and split) against the oracle's compat mode.

The rule, per scene and configuration: discrete + far segments <= 2 x the largest count of a one-ulp libm stand-in on that scene + 2; over
the sweep of one configuration <= 2 x the stand-ins' largest sweep total + one segment per 100 000 (lockstep.scene_cap / sweep_cap: computed
from the stand-in libraries at run time, nothing is typed in).  The first-hit depth of pass 0 is bit-equal — no libm call precedes the first
hit — except, in the compat modes with HIPRZ_COMPAT_SCATTERING, where the medium scattered the first segment: that depth is
-logf(u + 1e-4) / sigma, glibc's logf against ocml's, within rel 1e-6 (CUDA-compat section; the allowance of
test_cuda_compat_oracle_gpu.py, and the only one).  ray_count() and pass_count() equal the oracle's.

Run with -s for the per-configuration totals beside their caps; the measured figures are in DESIGN.md (Oracle, "Lockstep").
"""
import os

import numpy as np
import pytest

import generated_scenes as G
import lockstep
import oracle
from lockstep import bad
from rayzath_amd.engine import COMPAT_REPROJECTION, COMPAT_SCATTERING, TREE_DEVICE, TREE_DEVICE_SAH, Context
from test_shading_inputs_gpu import PACKAGINGS

pytestmark = pytest.mark.gpu

CHUNK = 10
CHUNKS = [G.SEEDS[i:i + CHUNK] for i in range(0, len(G.SEEDS), CHUNK)]
DERIVED_CHUNK = len(CHUNKS)   # run_chunk's index of generated_scenes.DERIVED, which is no part of the sweep's totals
CONFIGS = {name: dict(settings=settings) for name, settings in PACKAGINGS.items()}
CONFIGS["two-streams"] = dict(devices=[0, 0])
CONFIGS["tree-device"] = dict(settings=dict(tree=TREE_DEVICE))
CONFIGS["tree-device-sah"] = dict(settings=dict(tree=TREE_DEVICE_SAH))
for _mode in (31, 63):
    CONFIGS[f"compat{_mode}-fused"] = dict(mode=_mode, pipeline=0, settings=dict(mode=_mode, pipeline=0))
    CONFIGS[f"compat{_mode}-split"] = dict(mode=_mode, pipeline=1, settings=dict(mode=_mode))   # the default must resolve to the split pipeline
# what tests/test_packaging_sweep_gpu.py found to render other last bits than "compat31-split" (coloured shadow masks are products in the
# order a walk meets the crossed triangles; that file's VARIANTS say where): each order is held to the oracle here
CONFIGS["compat31-inline-shadows"] = dict(mode=31, pipeline=1, settings=dict(mode=31), env={"HIPRZ_DEFER_SHADOWS": "0"})
CONFIGS["compat31-shadow-beams"] = dict(mode=31, pipeline=1, settings=dict(mode=31), env={"HIPRZ_SHADOW_PACKET": "1"})
CONFIGS["compat31-tree-device-sah"] = dict(mode=31, pipeline=1, settings=dict(mode=31, tree=TREE_DEVICE_SAH))
_RESULTS = {}


def _context(config):
    saved = {k: os.environ.get(k) for k in config.get("env", {})}
    os.environ.update(config.get("env", {}))   # read by hiprz_create
    try:
        ctx = Context(config.get("devices", 0))
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    for k, v in config.get("settings", {}).items():
        getattr(ctx, "set_" + k)(v)
    return ctx


def _check_depth(result, seed, mode):
    """pass 0: bit-equal; a first segment the medium scattered (compat modes) within rel 1e-6"""
    depth, rdepth = result["depth"]
    if not mode & COMPAT_SCATTERING:
        assert result["depth_mismatch"] == 0, f"seed {seed}: first-hit depth differs on {result['depth_mismatch']} pixels"
        return
    flat, cam, cfg = lockstep.flat_scene(seed)[:3]
    plain = oracle.OracleRenderer(flat, cam, cfg, mode=mode & ~COMPAT_SCATTERING)
    plain.render(1, threads=1)
    unscattered = rdepth == plain.depth
    plain.close()
    assert np.array_equal(depth[unscattered], rdepth[unscattered]), f"seed {seed}: first-hit depth differs where nothing scattered"
    assert np.allclose(depth, rdepth, rtol=1e-6, atol=0), f"seed {seed}: scattered first-hit depth beyond rel 1e-6"


def run_chunk(name, chunk, counted=False):
    """one context, the chunk's scenes uploaded one after the other: {seed: lockstep result}; rendered once per (configuration, chunk)"""
    key = (name, chunk, counted)
    if key in _RESULTS:
        return _RESULTS[key]
    config, out = CONFIGS[name], {}
    mode = config.get("mode", 0)
    ctx = _context(config)
    for seed in (CHUNKS + [G.DERIVED])[chunk]:
        flat, cam, cfg = G.flat_scene(seed)[:3]
        if mode & COMPAT_REPROJECTION:
            # a context that keeps its frame size blends the previous scene's frame into pass 0 (hiprz_upload_camera drops the history on
            # a resize only) and the oracle has no history: every scene gets a context of its own, so mode 63 renders what mode 31 renders
            ctx.close()
            ctx = _context(config)
        ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
        ref = oracle.OracleRenderer(flat, cam, cfg, mode=mode)
        result = lockstep.lockstep(ctx, ref, G.PASSES, counted=counted)
        result["rays"] = (ctx.ray_count(), ref.traced_rays)
        result["passes"] = (ctx.pass_count(), ref.passes)
        result["pipeline"] = ctx.pipeline()
        ref.close()
        out[seed] = result
    ctx.close()
    _RESULTS[key] = out
    return out


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_lockstep_sweep(built, name, chunk):
    """Measured on MI355X, 337 440 segments per configuration: the default-mode configurations all show 314 300 exact, 1 far (seed 0, scene
    cap 6), 0 discrete against a sweep cap of 13; compat 31 / 63 show 285 827 (fused) / 285 805 (split) exact, 0 far, 0 discrete against
    13.  The sweep found one host bug: a part that owns no tile of the frame (seed 4, 1x1, on two streams, after seed 3) kept the previous
    frame's ray count."""
    mode = CONFIGS[name].get("mode", 0)
    results = run_chunk(name, chunk)
    failures = []
    for seed, r in results.items():
        cap = lockstep.scene_cap(seed, mode)
        print(f"lockstep {name} seed {seed}: {r['segments']} segments, exact {r['exact']}, far {r['far']}, discrete {r['discrete']}, cap {cap}")
        _check_depth(r, seed, mode)
        cam = G.flat_scene(seed)[1]
        assert r["rays"][0] == r["rays"][1] == G.PASSES * cam.width * cam.height, (seed, r["rays"])
        assert r["passes"][0] == r["passes"][1] == G.PASSES, (seed, r["passes"])
        if "pipeline" in CONFIGS[name]:
            assert r["pipeline"] == CONFIGS[name]["pipeline"], (seed, r["pipeline"])
        if bad(r) > cap:
            failures.append(f"seed {seed}: {r['discrete']} discrete + {r['far']} far segments, cap {cap}\n{lockstep.describe(r)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_lockstep_sweep_total(built, name):
    """the whole sweep of one configuration (the chunks above, rendered here if they were not yet)"""
    mode = CONFIGS[name].get("mode", 0)
    total = dict(segments=0, exact=0, far=0, discrete=0)
    worst = []
    for chunk in range(len(CHUNKS)):
        for seed, r in run_chunk(name, chunk).items():
            for k in total:
                total[k] += r[k]
            if bad(r):
                worst.append(f"seed {seed}: {r['discrete']} discrete + {r['far']} far\n{lockstep.describe(r)}")
    cap = lockstep.sweep_cap(G.SEEDS, mode)
    print(f"lockstep sweep {name}: {total['segments']} segments, exact {total['exact']}, far {total['far']}, discrete {total['discrete']}, "
          f"cap on far + discrete {cap}")
    assert total["far"] + total["discrete"] <= cap, "\n".join(worst)


@pytest.mark.parametrize("name", ["default", "compat31-split"])
def test_lockstep_derived_scenes(built, name):
    """The scenes without lights and without maps derived from sweep scenes (generated_scenes.DERIVED) under the per-scene rule above, in
    the two configurations whose pass-by-pass renders are the baselines of tests/test_packaging_sweep_gpu.py: that file's bit-equalities
    carry this comparison to every other packaging on these scenes too."""
    mode = CONFIGS[name].get("mode", 0)
    failures = []
    for seed, r in run_chunk(name, DERIVED_CHUNK).items():
        cap = lockstep.scene_cap(seed, mode)
        print(f"lockstep {name} scene {seed}: {r['segments']} segments, exact {r['exact']}, far {r['far']}, discrete {r['discrete']}, cap {cap}")
        _check_depth(r, seed, mode)
        cam = G.flat_scene(seed)[1]
        assert r["rays"][0] == r["rays"][1] == G.PASSES * cam.width * cam.height, (seed, r["rays"])
        assert r["passes"][0] == r["passes"][1] == G.PASSES, (seed, r["passes"])
        if bad(r) > cap:
            failures.append(f"scene {seed}: {r['discrete']} discrete + {r['far']} far segments, cap {cap}\n{lockstep.describe(r)}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(PACKAGINGS))
def test_lockstep_counters(built, name):
    """The sweep's first 10 scenes through render_counted(1) — the instrumented instantiations — in lockstep: the rule above, and every
    pass's work counters against the oracle's from the same inputs, the keys and the way test_shading_inputs_against_the_oracle compares
    them on its first pass (segments, hits, light samples, finished paths, closest-hit box and triangle tests, texel fetches equal; shadow
    rays within 2, none without lights)."""
    failures = []
    for seed, r in run_chunk(name, 0, counted=True).items():
        world = G.flat_scene(seed)[3]
        lights = bool(world.spot_lights or world.direct_lights)
        assert r["depth_mismatch"] == 0, seed
        if bad(r) > lockstep.scene_cap(seed):
            failures.append(f"seed {seed}: {r['discrete']} discrete + {r['far']} far segments, cap {lockstep.scene_cap(seed)}\n{lockstep.describe(r)}")
        for p, (dev, ref) in enumerate(r["counters"]):
            for k in ("segments", "hits", "light_samples", "finished", "texel_fetches"):
                assert dev[k] == ref[k], (seed, p, k, dev[k], ref[k])
            for total, shadow in (("box_tests", "shadow_box_tests"), ("tri_tests", "shadow_tri_tests")):
                assert dev[total] - dev[shadow] == ref[total] - ref[shadow], (seed, p, total)
            if lights:
                assert abs(dev["shadow_rays"] - ref["shadow_rays"]) <= 2, (seed, p, dev["shadow_rays"], ref["shadow_rays"])
            else:
                assert dev["shadow_rays"] == 0 == dev["light_samples"], (seed, p)
    assert not failures, "\n".join(failures)


def test_part_without_tiles_restarts_its_ray_count(built):
    """A part of a two-stream context that owns no tile of the frame (1x1: one tile, the first part's) restarts its ray counter with the
    frame: after a 64x3 frame (96 pixels each, 8 passes) the 1x1 frame's 8 passes are 8 rays, not 8 + 768."""
    ctx = Context([0, 0])
    for seed in (3, 4):   # 64x3, then 1x1
        flat, cam, cfg = G.flat_scene(seed)[:3]
        assert (cam.width, cam.height) == G.SIZES[seed]
        ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
        ctx.render(1), ctx.render(G.PASSES - 1)
        assert ctx.ray_count() == G.PASSES * cam.width * cam.height, seed
    ctx.close()
