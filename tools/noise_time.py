#!/usr/bin/env python3
"""Device time of a noise measurement (Context.noise: include/hiprz_noise.h) beside the step of the frame it measures, with the variance
estimate on: the median of `--repeats` measurements, HIP events on the context's stream.

    python tools/noise_time.py --config B --out profiles/r15/noise_time_B.json

A measurement is split into the assembly of the two row-major images (hiprz_accum_device + hiprz_variance_device: untile kernels and
rz_variance_kernel, libhiprz.so) and the tile kernel (hiprz_noise_tiles into a device buffer: rz_noise_tiles_kernel alone, libhiprz_noise.so);
the whole Context.noise() call — assembly, kernel, copy of the tile records to pinned memory, stream wait, host summary — is timed by the
host's clock."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayzath_amd import _hiprt, noise, scenes  # noqa: E402
from rayzath_amd.engine import Context, RenderConfig, Tracing  # noqa: E402
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
    ctx.set_variance(1)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(preset["max_depth"], args.passes)).struct())
    ctx.render(1)
    for _ in range(8):
        ctx.render(args.passes)
    ctx.sync()
    step = timed(ctx, lambda: ctx.render(args.passes), args.repeats)
    summary, _ = ctx.noise()  # allocations, first launch
    assembly = timed(ctx, lambda: (ctx.accum_device(), ctx.variance_device()), args.repeats)
    tx, ty = noise.tile_grid(W, H)
    out = _hiprt.DeviceBuffer(tx * ty * 16)
    accum, variance = ctx.accum_device(), ctx.variance_device()
    params = noise.Params(cam.aperture, cam.exposure_time, 1.0 / 255.0, 8)
    kernel = timed(ctx, lambda: ctx._meter.tiles(accum, variance, W, H, params, out.ptr, ctx.stream()), args.repeats)
    calls = []
    for _ in range(args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        summary, _ = ctx.noise()
        calls.append((time.perf_counter() - t0) * 1.0e3)
    out.free()
    ctx.close()
    result = {"config": args.config, "width": W, "height": H, "label": args.label, "tiles": tx * ty, "passes_per_step": args.passes,
              "ms_per_step_variance": step[0], "ms_per_step_variance_min": step[1],
              "assembly_ms": assembly[0], "assembly_ms_min": assembly[1], "tile_kernel_ms": kernel[0], "tile_kernel_ms_min": kernel[1],
              "noise_call_host_ms": statistics.median(calls), "noise_call_host_ms_min": min(calls),
              "bytes_read": 2 * 16 * W * H, "bytes_written": 16 * tx * ty, "repeats": args.repeats,
              "rms": summary.rms, "tile_rms_max": summary.tile_rms_max, "estimated": summary.estimated, "pixels": summary.pixels}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
