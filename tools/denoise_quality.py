#!/usr/bin/env python3
"""Error of the denoised frame over a grid of filter parameters: the measurements the default hiprz_denoise_params were taken from.

For the two scenes of the quality test (tests/test_denoise_gpu.py: the Cornell box, and the preset with lights and maps) at WIDTH x HEIGHT:
a frame of N = 64 passes and a reference of 64 * N passes on another seed; per parameter set the RMSE, over the tone-mapped image in
[0, 1] before quantisation, of the denoised N-pass frame and of the denoised reference against the reference, and their ratios to the raw
N-pass frame's RMSE (both must stay below 1).

    python tools/denoise_quality.py 960 540 > profiles/r07/quality_sweep_960x540.txt
    python tools/denoise_quality.py 256 192 --all > profiles/r07/quality_sweep_256x192.txt     (--all: iterations, sigma_normal and sigma_depth too)
    python tools/denoise_quality.py 960 540 --variance > profiles/r08/quality_sweep_variance.txt

--variance: the N-pass frame is rendered as 8 calls of N / 8 passes (the batches of hiprz_set_variance; the accumulator's bits do not
depend on how the passes are split into calls) and the variance-guided filter (HIPRZ_DENOISE_VARIANCE) is swept over sigma_color = 1, 2,
4, 8, 16 standard deviations next to the sweep above, on the same frames."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_reference as ref  # noqa: E402
from rayzath_amd import scenes  # noqa: E402
from rayzath_amd.engine import Context, LightSampling, RenderConfig, Tracing, denoise_params  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--all", action="store_true", help="sweep iterations, sigma_normal and sigma_depth beside sigma_color")
    ap.add_argument("--variance", action="store_true", help="also sweep the variance-guided filter over sigma_color 1, 2, 4, 8, 16 (frame rendered as 8 calls)")
    args = ap.parse_args()
    W, H, N = args.width, args.height, args.passes
    presets = {"cornell": (lambda: scenes.cornell_box(W, H), LightSampling()),
               "lights and maps": (lambda: scenes.shading_inputs_scene(W, H, lights=True), LightSampling(2, 2))}
    colors = (0.0, 0.1, 0.25, 0.35, 0.5, 0.7, 1.0, 1.5, 2.0, 4.0)
    grid = list(itertools.product((4, 5), (32.0, 128.0), (0.02, 0.1, 0.5), colors) if args.all else itertools.product((5,), (128.0,), (0.1,), colors))
    print(f"{W} x {H}, {N}-pass frame against {64 * N} passes")
    for name, (build, sampling) in presets.items():
        world = build()
        noisy, clean = Context(0), Context(0)
        for ctx, seed in ((noisy, 20240501), (clean, 977)):
            flat, cam = flatten(world), camera_struct(world.camera)
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(sampling, Tracing(8, N), seed=seed).struct())
            ctx.set_variance(args.variance)
        for calls in ([N // 8] * 8 if args.variance else [N]):
            noisy.render(calls)
        for _ in range(64):
            clean.render(N)
        tm = lambda image: ref.tonemap_unquantised(image, cam.aperture, cam.exposure_time)  # noqa: E731
        reference = tm(clean.read_accum())
        raw = rmse(tm(noisy.read_accum()), reference)
        print(f"{name}: raw {raw:.5f}", flush=True)
        for it, sn, sz, sc in grid:
            p = denoise_params(iterations=it, sigma_normal=sn, sigma_depth=sz, sigma_color=sc)
            noisy.denoise(p), clean.denoise(p)
            d, b = rmse(tm(noisy.read_denoised()), reference), rmse(tm(clean.read_denoised()), reference)
            print(f"  iterations {it} sigma_normal {sn:5.0f} sigma_depth {sz:4.2f} sigma_color {sc:4.2f}: denoised {d:.5f} ({d / raw:.3f} of raw)  "
                  f"denoised reference {b:.5f} ({b / raw:.3f} of raw)", flush=True)
        for sc in ((1.0, 2.0, 4.0, 8.0, 16.0) if args.variance else ()):
            p = denoise_params(sigma_color=sc, variance=True)
            noisy.denoise(p), clean.denoise(p)
            d, b = rmse(tm(noisy.read_denoised()), reference), rmse(tm(clean.read_denoised()), reference)
            print(f"  variance-guided, iterations {p.iterations} sigma_normal {p.sigma_normal:5.0f} sigma_depth {p.sigma_depth:4.2f} sigma_color {sc:5.2f} sd: "
                  f"denoised {d:.5f} ({d / raw:.3f} of raw)  denoised reference {b:.5f} ({b / raw:.3f} of raw)", flush=True)
        noisy.close(), clean.close()


if __name__ == "__main__":
    main()
