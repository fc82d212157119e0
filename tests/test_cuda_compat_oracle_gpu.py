"""The CUDA-compat integrator (hiprz_set_mode) pixel by pixel against the CPU oracle's compat mode (rzo_render_pass_mode, oracle/rz_oracle.c:
a restatement of the reference's CUDA text, not of hiprz_compat.hpp), the way the default mode is checked against the oracle's CPU mode.

  scenes     compat_showcase (tests/compat_common.py: coloured partly transparent textured sheets between a spot and a direct light and the
             receivers, tinted absorbing glass, a scattering world medium and a scattering object, RGBA8 / R8 / R32F maps under every filter x
             address mode on transforms that leave [0, 1]), scenes.living_room(96, 64, 16), scenes.shading_inputs_scene(96, 64), and
             open_sky (a mapped sky seen from outside the world's root box; flags 8, 16, 63 only)
  flags      1, 2, 4, 8, 16, 31, 59, 63 on the fused kernel (hiprz_set_pipeline(0): rz_compat_pass_kernel) and on the default split pipeline
             (sorted rays, rz_trace_coop_compat_kernel, rz_shade_kernel<.., RZ_SHADOW_COMPAT_DEFER>, the mask-collecting shadow kernels);
             4 and 63 also with HIPRZ_SHADOW_PACKET=1 / 0 (both mask walks, whatever the auto rule picks) and under HIPRZ_TREE_AUTO
  passes     one counted first pass, 8, then 3, at depth 5: paths reach the depth limit and restart with regenerated rays
  full size  config E (living room 3840x2160) in modes 59 and 63 on the shipped packaging (HIPRZ_TREE_AUTO, default streams), 12 passes

What the two sides legitimately differ in is glibc-vs-ocml libm (logf of the scattering distance, powf of Beer-Lambert, and the sinf / cosf /
powf / expf of mode 0): an ulp moves a path across an edge.  And on the split pipeline the coloured masks are the same factors multiplied
in another order (the deferred kernels multiply front to back over a quad of testers and check the 1e-4 early-out on one running mask,
cuda_bvh.cuh groups per instance): rgb to rounding, the mask's texel fetches where a mask falls below 1e-4.  Measured figures are in the
docstrings of the tests; every threshold is the measured value minus a margin.
"""
import numpy as np
import pytest

import oracle
from compat_common import compat_showcase, open_sky
from rayzath_amd import scenes
from rayzath_amd.engine import COMPAT_SCATTERING, TREE_AUTO, Context, LightSampling, RenderConfig, Tracing, default_streams
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

DEPTH = 5
SCENES = {"showcase": (lambda: compat_showcase(160, 96), (1, 1)),
          "living_room": (lambda: scenes.living_room(96, 64, 16), (2, 1)),
          "shading_inputs": (lambda: scenes.shading_inputs_scene(96, 64), (1, 2)),
          "open_sky": (lambda: open_sky(96, 64), (1, 1))}
FLAGS = [1, 2, 4, 8, 16, 31, 59, 63]
NON_SHADOW = ("segments", "hits", "light_samples", "finished")
_FLAT, _ORACLE = {}, {}


def scene(name):
    if name not in _FLAT:
        build, samples = SCENES[name]
        world = build()
        _FLAT[name] = (flatten(world), camera_struct(world.camera), RenderConfig(LightSampling(*samples), Tracing(DEPTH, 8)).struct())
    return _FLAT[name]


def oracle_frame(name, flags):
    """1 counted + 8 + 3 passes in the oracle, once per (scene, flags)."""
    if (name, flags) not in _ORACLE:
        flat, cam, cfg = scene(name)
        ref = oracle.OracleRenderer(flat, cam, cfg, mode=flags)
        first = ref.render(1, counted=True)
        ref.render(8), ref.render(3)
        _ORACLE[name, flags] = dict(first=first, accum=ref.accum, depth=ref.depth)
        ref.close()
    return _ORACLE[name, flags]


def gpu_frame(name, flags, packaging, monkeypatch):
    flat, cam, cfg = scene(name)
    if packaging in ("packet", "coop"):
        monkeypatch.setenv("HIPRZ_SHADOW_PACKET", "1" if packaging == "packet" else "0")
    ctx = Context(0)
    ctx.set_mode(flags)
    if packaging == "fused":
        ctx.set_pipeline(0)
    if packaging == "auto_tree":
        ctx.set_tree(TREE_AUTO)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    first = ctx.render_counted(1)
    ctx.render(8), ctx.render(3)
    out = dict(first=first, accum=ctx.read_accum(), depth=ctx.read_depth(), pipeline=ctx.pipeline())
    ctx.close()
    return out


def compare(gpu, ref):
    acc, racc = gpu["accum"], ref["accum"]
    close = (np.abs(acc[..., :3] - racc[..., :3]) <= 1e-3 * np.maximum(np.abs(racc[..., :3]), 1.0)).all(-1).mean()
    return close, (acc[..., 3] == racc[..., 3]).mean()


RUNS = [(f, p) for f in FLAGS for p in ("fused", "split")] + [(f, p) for f in (4, 63) for p in ("packet", "coop", "auto_tree")]
# the mapped sky seen from outside the scene's bounds: the flags that read maps
SKY_RUNS = [(f, p) for f in (8, 16, 63) for p in ("fused", "split")]
# (rgb within 1e-3, finished-path counts equal) per scene: the measured minimum over all 22 runs minus a margin
LIT = {"showcase": (0.988, 0.9995), "living_room": (0.988, 0.9995), "shading_inputs": (0.9999, 0.9999), "open_sky": (0.999, 0.9999)}


@pytest.mark.parametrize("name,flags,packaging", [(n, f, p) for f, p in RUNS for n in SCENES if n != "open_sky"] +
                         [("open_sky", f, p) for f, p in SKY_RUNS])
def test_compat_frame_against_the_oracle(built, monkeypatch, name, flags, packaging):
    """First-hit depth equal (a first segment the medium scattered ends at -logf(u + 1e-4) / sigma: glibc's and ocml's logf, within 1e-6);
    the counted first pass's segments, hits, light samples and finished paths equal on every packaging, and on the fused kernel with the
    reference trees every counter (its mask walk groups per instance as cuda_bvh.cuh does, so it stops where the oracle stops: texel fetches
    and shadow counters equal too); the accumulator's finished-path counts equal and its rgb within 1e-3 on the shares of LIT.
    Elsewhere the closest-hit and shadow box / triangle counts differ (the sorted pipeline's front-to-back walk visits other nodes) and the
    texel fetches may (the deferred mask kernels check the 1e-4 early-out on one running mask: shading_inputs 9718 against 9712).
    open_sky: a mapped sky that most primary rays meet outside the world's root box (calculateTexcrd on every miss).
    Measured on MI355X (rgb within 1e-3 / finished paths equal, the same on every packaging of a flag set):
      showcase        1: 0.99850  2: 0.99798  4: 0.99193  8: 0.99746  16: 0.99837  31, 63: 0.99004  59: 0.99818  alpha 1.0 everywhere
      living_room     0.99365 (1, 2, 8, 16, 59), 0.99040 (4, 31, 63)  alpha 0.99984
      shading_inputs  1.0 / 1.0 everywhere
      open_sky        1.0 / 1.0 everywhere
    The shadow-colour flag lowers the share: light now passes the sheets and glass, so more pixels carry the libm-dependent terms of a
    light sample.  An oracle whose sinf / cosf / acosf / powf / expf / logf each return one ulp less gives the same picture against the
    oracle: showcase 0.99447 (mode 0), 0.98398 (4), 0.98255 (63); living_room 0.96973 (0), 0.96240 (4).  The pixels the GPU disagrees on
    are mostly ones such an oracle moves: with one ulp down, one up and one of the two chosen per argument, showcase 1: 23 of 23, 4: 103
    of 124; living_room 1: 34 of 39, 4 and 63: 54 of 59."""
    ref, gpu = oracle_frame(name, flags), gpu_frame(name, flags, packaging, monkeypatch)
    assert gpu["pipeline"] == (0 if packaging == "fused" else 1)
    if flags & COMPAT_SCATTERING:
        unscattered = ref["depth"] == oracle_frame(name, flags & ~COMPAT_SCATTERING)["depth"]
        assert np.array_equal(gpu["depth"][unscattered], ref["depth"][unscattered])
        assert np.allclose(gpu["depth"], ref["depth"], rtol=1e-6, atol=0)
    else:
        assert np.array_equal(gpu["depth"], ref["depth"])
    first, rfirst = gpu["first"], ref["first"]
    for k in NON_SHADOW:
        assert first[k] == rfirst[k], k
    if packaging == "fused":
        assert first == rfirst
    else:   # the deferred mask kernels' early-out on the running mask: a few fetches more or fewer (shading_inputs: 6 in 9712)
        assert abs(first["texel_fetches"] - rfirst["texel_fetches"]) <= 2e-3 * rfirst["texel_fetches"]
    close, alpha = compare(gpu, ref)
    print(f"compat {name} flags {flags} {packaging}: rgb within 1e-3 {close:.6f}, alpha equal {alpha:.6f}, texel fetches "
          f"{first['texel_fetches']} / {rfirst['texel_fetches']}, shadow rays {first['shadow_rays']} / {rfirst['shadow_rays']}")
    assert ref["accum"][..., 3].max() >= 2.0
    assert close >= LIT[name][0] and alpha >= LIT[name][1]


_FULL = {}


@pytest.mark.parametrize("flags,rgb_close,alpha_equal", [(59, 0.993, 0.9995), (63, 0.989, 0.9995)])
def test_config_e_full_size_compat_against_the_oracle(built, flags, rgb_close, alpha_equal):
    """Config E at 3840x2160, the packaging that ships (HIPRZ_TREE_AUTO on engine.default_streams streams: sorted rays, the compat trace,
    deferred shade and mask kernels), 12 passes at depth 8 against the oracle's compat mode.  Measured on MI355X: mode 59 0.99376 within
    1e-3, finished paths 0.99959 equal; mode 63 0.99067 / 0.99959 (mode 0, test_full_size_gpu.py: 0.9938 / 0.9996).  Mode 63's rgb bar is
    below mode 0's 0.992: the coloured masks let the lights through glass and fog, and each such light sample is one more libm-dependent
    term (the one-ulp oracle of test_compat_frame_against_the_oracle's docstring moves E's mode 63 more than its mode 0 too).
    The oracle takes about 14 s per mode at 4K on 16 cores."""
    import time
    preset = scenes.CONFIGS["E"]
    world = preset["build"]()
    flat, cam, depth = flatten(world), camera_struct(world.camera), preset["max_depth"]
    cfg = RenderConfig(tracing=Tracing(depth, 8)).struct()
    t = time.time()
    ref = oracle.OracleRenderer(flat, cam, cfg, mode=flags)
    ref.render(1), ref.render(8), ref.render(3)
    racc, rdepth = ref.accum, ref.depth
    ref.close()
    oracle_s = time.time() - t
    k = default_streams(len(flat.spot_lights) + len(flat.direct_lights))
    ctx = Context([0] * k) if k > 1 else Context(0)
    ctx.set_mode(flags), ctx.set_tree(TREE_AUTO)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    ctx.render(1), ctx.render(8), ctx.render(3)
    acc = ctx.read_accum()
    assert np.array_equal(ctx.read_depth(), rdepth)
    close = (np.abs(acc[..., :3] - racc[..., :3]) <= 1e-3 * np.maximum(np.abs(racc[..., :3]), 1.0)).all(-1).mean()
    alpha = (acc[..., 3] == racc[..., 3]).mean()
    print(f"config E compat {flags}: oracle {oracle_s:.1f} s, rgb within 1e-3 {close:.6f}, alpha equal {alpha:.6f}")
    assert racc[..., 3].max() >= 2.0
    assert close >= rgb_close and alpha >= alpha_equal
    ctx.close()
