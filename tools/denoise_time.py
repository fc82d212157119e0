#!/usr/bin/env python3
"""Device time of the denoiser beside the frame it filters: the guide kernel, the a-trous filter (default parameters) and one bench step
(8 passes) of the same scene, each as the median of `--repeats` measurements with HIP events on the context's stream.

    python tools/denoise_time.py --config B --out profiles/r07/denoise_time_B.json

The filter is timed through hiprz_denoise_image on the context's own guides (filter alone) and through hiprz_denoise (guides when stale,
assembly, filter, tone map: what a frame pays).  Then the same with hiprz_set_variance on: the step again (its difference to the first
is rz_moments_kernel, once per call: reported against the mean of a step before and a step after with the estimate off), the assembly
of the estimate (hiprz_variance_device) and the variance-guided filter through hiprz_denoise_image_variance."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import _hiprt, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing, denoise_params  # noqa: E402
from rayzath_amd.scene import camera_struct, flatten  # noqa: E402


def timed(ctx, fn, repeats):
    a, b = _hiprt.Event(), _hiprt.Event()
    out = []
    for _ in range(repeats):
        a.record(ctx.stream())
        fn()
        b.record(ctx.stream())
        out.append(b.ms_since(a))
    a.destroy(), b.destroy()
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--passes", type=int, default=8, help="passes of a step (bench.py: 8)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    preset = scenes.CONFIGS[args.config]
    world = preset["build"]()
    flat, cam = flatten(world), camera_struct(world.camera)
    W, H = cam.width, cam.height
    ctx = Context(0)
    ctx.set_tree(4)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], args.passes)).struct())
    ctx.render(1)
    for _ in range(5):
        ctx.render(args.passes)
    ctx.sync()
    step = timed(ctx, lambda: ctx.render(args.passes), args.repeats)
    params = denoise_params()
    ctx.denoise(params)  # allocations, first launches
    ctx.sync()
    guides = timed(ctx, ctx.render_guides, args.repeats)
    accum = _hiprt.DeviceBuffer.of(ctx.read_accum())
    dst = _hiprt.DeviceBuffer(W * H * 16)
    ctx.denoise_image(accum.ptr, None, params, dst.ptr)
    ctx.sync()
    filt = timed(ctx, lambda: ctx.denoise_image(accum.ptr, None, params, dst.ptr), args.repeats)
    whole = timed(ctx, lambda: ctx.denoise(params), args.repeats)
    checksum = float(np.float64(dst.download((H, W, 4), np.float32)[..., :3]).sum())
    # the same context with the estimate on (a restart: warmed up again), steps interleaved with the plain ones' figure above
    ctx.set_variance(1)
    ctx.render(1)
    for _ in range(5):
        ctx.render(args.passes)
    ctx.sync()
    step_v = timed(ctx, lambda: ctx.render(args.passes), args.repeats)
    estimate = timed(ctx, ctx.variance_device, args.repeats)
    flagged = denoise_params(variance=True, sigma_color=4.0)
    variance = _hiprt.DeviceBuffer.of(ctx.read_variance())
    ctx.denoise_image_variance(accum.ptr, None, variance.ptr, flagged, dst.ptr)
    ctx.sync()
    filt_v = timed(ctx, lambda: ctx.denoise_image_variance(accum.ptr, None, variance.ptr, flagged, dst.ptr), args.repeats)
    whole_v = timed(ctx, lambda: ctx.denoise(flagged), args.repeats)
    ctx.set_variance(0)
    ctx.render(1)
    for _ in range(5):
        ctx.render(args.passes)
    ctx.sync()
    step_again = timed(ctx, lambda: ctx.render(args.passes), args.repeats)
    accum.free(), dst.free(), variance.free()
    ctx.close()
    result = {"config": args.config, "width": W, "height": H, "label": args.label, "iterations": params.iterations,
              "ms_per_step": step[0], "ms_per_step_min": step[1], "passes_per_step": args.passes,
              "guide_kernel_ms": guides[0], "guide_kernel_ms_min": guides[1],
              "filter_ms": filt[0], "filter_ms_min": filt[1], "denoise_call_ms": whole[0], "denoise_call_ms_min": whole[1],
              "ms_per_step_variance": step_v[0], "ms_per_step_variance_min": step_v[1], "ms_per_step_off_again": step_again[0],
              "moments_kernel_ms": step_v[0] - 0.5 * (step[0] + step_again[0]),
              "variance_assembly_ms": estimate[0], "variance_assembly_ms_min": estimate[1],
              "variance_filter_ms": filt_v[0], "variance_filter_ms_min": filt_v[1], "variance_denoise_call_ms": whole_v[0],
              "repeats": args.repeats, "checksum": checksum}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
